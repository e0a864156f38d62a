# conn_asan: the host entries of the local-map store under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its
# own (never loaded into python, never run on a GPU: the store has no context).  Not part of build(); run by hand:
#   make -C tests/native -f conn_asan.mk && tests/native/conn_asan
# lmap_store.cpp, lmap.cpp and lmap_conn.cpp are compiled into the program with the sanitizers on its host side; the two kernel files
# only satisfy their launch symbols.
ROOT := $(abspath ../..)
SRC := $(ROOT)/dr_slam_amd/csrc
HIPCC ?= /opt/rocm/bin/hipcc
FLAGS := -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Wall -I$(ROOT)/include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer

all: conn_asan

conn_asan: conn_asan.cpp $(SRC)/lmap_store.cpp $(SRC)/lmap.cpp $(SRC)/lmap_conn.cpp $(SRC)/lmap_store.h $(SRC)/lmap_call.h $(SRC)/resident_block.h $(SRC)/lmap_kernels.hip $(SRC)/conn_kernels.hip $(SRC)/conn_core.h $(SRC)/lmap_core.h $(SRC)/lmap_internal.h $(SRC)/lmap_device.h
	$(HIPCC) $(FLAGS) -x hip conn_asan.cpp $(SRC)/lmap_store.cpp $(SRC)/lmap.cpp $(SRC)/lmap_conn.cpp $(SRC)/lmap_kernels.hip $(SRC)/conn_kernels.hip -o $@

clean:
	rm -f conn_asan
