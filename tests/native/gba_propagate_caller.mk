# The native caller of the map update after a global bundle adjustment (built by __graft_entry__.build() next to the callers of Makefile):
# Planar_SLAM::LocalMapTracker::PropagateGlobalBA over stand-in classes next to a pointer-walking restatement of src/LoopClosing.cc:722-783.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: gba_propagate_caller

gba_propagate_caller: gba_propagate_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f gba_propagate_caller
