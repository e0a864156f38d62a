# essential_asan: essential_caller.cpp with the local-map store's host code compiled into it under AddressSanitizer and
# UndefinedBehaviorSanitizer, as a program of its own (never loaded into python, never run on a GPU: run it in host mode, where the
# store has no context).  Not part of build(); tests/test_essential_cpu.py builds and runs it:
#   make -C tests/native -f essential_asan.mk && tests/native/essential_asan host
# lmap_store.cpp, lmap.cpp, lmap_conn.cpp, lmap_correct.cpp (the geometry both calls read) and lmap_essential.cpp are compiled into
# the program with the sanitizers on its host side; the kernel files only satisfy their launch symbols, and libdrfe.so the
# adaptor's references to the other entries, which host mode never calls.
ROOT := $(abspath ../..)
SRC := $(ROOT)/dr_slam_amd/csrc
HIPCC ?= /opt/rocm/bin/hipcc
FLAGS := -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Wall -I$(ROOT)/include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
LDFLAGS := -L$(SRC) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib
HOST := $(SRC)/lmap_store.cpp $(SRC)/lmap.cpp $(SRC)/lmap_conn.cpp $(SRC)/lmap_correct.cpp $(SRC)/lmap_essential.cpp
KERNELS := $(SRC)/lmap_kernels.hip $(SRC)/conn_kernels.hip $(SRC)/correct_kernels.hip $(SRC)/essential_kernels.hip

all: essential_asan

essential_asan: essential_caller.cpp $(HOST) $(KERNELS) $(SRC)/lmap_store.h $(SRC)/lmap_call.h $(SRC)/resident_block.h $(SRC)/essential_core.h $(SRC)/lmap_internal.h $(ROOT)/include/drfe_adaptor.hpp
	$(HIPCC) $(FLAGS) -x hip essential_caller.cpp $(HOST) $(KERNELS) -o $@ $(LDFLAGS)

clean:
	rm -f essential_asan
