# insert_asan: the host entry of the item loops of ProcessNewKeyFrame under AddressSanitizer and UndefinedBehaviorSanitizer, as a
# program of its own (never loaded into python, never run on a GPU: the stores have no context).  Not part of build(); run by hand:
#   make -C tests/native -f insert_asan.mk && tests/native/insert_asan
# lmap_store.cpp, lmap.cpp, lmap_correct.cpp, lmap_cull.cpp, lmap_recent.cpp and lmap_insert.cpp are compiled into the program with
# the sanitizers on its host side; the kernel files only satisfy their launch symbols, and libdrfe.so the references to the context
# entries, which a host-only store never calls.
ROOT := $(abspath ../..)
SRC := $(ROOT)/dr_slam_amd/csrc
HIPCC ?= /opt/rocm/bin/hipcc
FLAGS := -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Wall -I$(ROOT)/include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
LDFLAGS := -L$(SRC) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib
HOST := $(SRC)/lmap_store.cpp $(SRC)/lmap.cpp $(SRC)/lmap_correct.cpp $(SRC)/lmap_cull.cpp $(SRC)/lmap_recent.cpp $(SRC)/lmap_insert.cpp
KERNELS := $(SRC)/lmap_kernels.hip $(SRC)/correct_kernels.hip $(SRC)/cull_kernels.hip $(SRC)/recent_kernels.hip $(SRC)/insert_kernels.hip

all: insert_asan

insert_asan: insert_asan.cpp $(HOST) $(KERNELS) $(SRC)/lmap_store.h $(SRC)/lmap_call.h $(SRC)/resident_block.h $(SRC)/insert_core.h $(SRC)/lmap_internal.h $(ROOT)/include/drfe.h
	$(HIPCC) $(FLAGS) -x hip insert_asan.cpp $(HOST) $(KERNELS) -o $@ $(LDFLAGS)

clean:
	rm -f insert_asan
