# cull_asan: the host entry of LocalMapping::KeyFrameCulling under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of
# its own (never loaded into python, never run on a GPU: the stores have no context).  Not part of build(); run by hand:
#   make -C tests/native -f cull_asan.mk && tests/native/cull_asan
# lmap_store.cpp, lmap.cpp, lmap_conn.cpp and lmap_cull.cpp are compiled into the program with the sanitizers on its host side; the kernel files only satisfy their
# launch symbols, and libdrfe.so the adaptor's references to the context entries, which a host-only store never calls.
ROOT := $(abspath ../..)
SRC := $(ROOT)/dr_slam_amd/csrc
HIPCC ?= /opt/rocm/bin/hipcc
FLAGS := -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Wall -I$(ROOT)/include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
LDFLAGS := -L$(SRC) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: cull_asan

cull_asan: cull_asan.cpp cull_caller.cpp $(SRC)/lmap_store.cpp $(SRC)/lmap.cpp $(SRC)/lmap_conn.cpp $(SRC)/lmap_cull.cpp $(SRC)/lmap_store.h $(SRC)/lmap_call.h $(SRC)/resident_block.h $(SRC)/lmap_kernels.hip $(SRC)/conn_kernels.hip $(SRC)/cull_kernels.hip $(SRC)/cull_core.h $(SRC)/lmap_internal.h $(ROOT)/include/drfe_adaptor.hpp
	$(HIPCC) $(FLAGS) -x hip cull_asan.cpp $(SRC)/lmap_store.cpp $(SRC)/lmap.cpp $(SRC)/lmap_conn.cpp $(SRC)/lmap_cull.cpp $(SRC)/lmap_kernels.hip $(SRC)/conn_kernels.hip $(SRC)/cull_kernels.hip -o $@ $(LDFLAGS)

clean:
	rm -f cull_asan
