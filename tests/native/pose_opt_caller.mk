# The native caller of PoseOptimization (built by __graft_entry__.build() next to the callers of Makefile):
# Planar_SLAM::Optimizer::PoseOptimization with the reference's signature and drfe::PoseOptBatch over stand-in frames.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: pose_opt_caller

pose_opt_caller: pose_opt_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f pose_opt_caller
