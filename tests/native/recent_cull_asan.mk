# recent_cull_asan: the host entry of LocalMapping::MapPointCulling and MapLineCulling under AddressSanitizer and
# UndefinedBehaviorSanitizer, as a program of its own (never loaded into python, never run on a GPU: the stores have no context).
# Not part of build(); run by hand:
#   make -C tests/native -f recent_cull_asan.mk && tests/native/recent_cull_asan
# lmap_store.cpp, lmap.cpp, lmap_cull.cpp and lmap_recent.cpp are compiled into the program with the sanitizers on its host side;
# the kernel files only satisfy their launch symbols, and libdrfe.so the adaptor's references to the context entries, which a
# host-only store never calls.
ROOT := $(abspath ../..)
SRC := $(ROOT)/dr_slam_amd/csrc
HIPCC ?= /opt/rocm/bin/hipcc
FLAGS := -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Wall -I$(ROOT)/include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
LDFLAGS := -L$(SRC) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib
HOST := $(SRC)/lmap_store.cpp $(SRC)/lmap.cpp $(SRC)/lmap_cull.cpp $(SRC)/lmap_recent.cpp
KERNELS := $(SRC)/lmap_kernels.hip $(SRC)/cull_kernels.hip $(SRC)/recent_kernels.hip

all: recent_cull_asan

recent_cull_asan: recent_cull_asan.cpp recent_cull_caller.cpp $(HOST) $(KERNELS) $(SRC)/lmap_store.h $(SRC)/lmap_call.h $(SRC)/resident_block.h $(SRC)/recent_core.h $(SRC)/lmap_internal.h $(ROOT)/include/drfe_adaptor.hpp
	$(HIPCC) $(FLAGS) -x hip recent_cull_asan.cpp $(HOST) $(KERNELS) -o $@ $(LDFLAGS)

clean:
	rm -f recent_cull_asan
