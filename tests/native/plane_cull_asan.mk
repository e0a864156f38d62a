# plane_cull_asan: the host entry of LocalMapping::MapPlaneCulling under AddressSanitizer and UndefinedBehaviorSanitizer, as a
# program of its own (never loaded into python, never run on a GPU: no context is created).  Not part of build(); run by hand:
#   make -C tests/native -f plane_cull_asan.mk && tests/native/plane_cull_asan
# plane_cull.cpp is compiled into the program with the sanitizers on its host side; libdrfe.so satisfies the launch symbols, the
# rounds of map_plane.cpp and the voxel grid (planes_post.cpp, not instrumented), none of which a call without a context reaches
# but the last.
ROOT := $(abspath ../..)
SRC := $(ROOT)/dr_slam_amd/csrc
HIPCC ?= /opt/rocm/bin/hipcc
FLAGS := -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Wall -I$(ROOT)/include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
LDFLAGS := -L$(SRC) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: plane_cull_asan

plane_cull_asan: plane_cull_asan.cpp plane_cull_caller.cpp $(SRC)/plane_cull.cpp $(SRC)/plane_cull_core.h $(SRC)/plane_map_internal.h $(ROOT)/include/drfe_adaptor.hpp
	$(HIPCC) $(FLAGS) -x hip plane_cull_asan.cpp $(SRC)/plane_cull.cpp -o $@ $(LDFLAGS)

clean:
	rm -f plane_cull_asan
