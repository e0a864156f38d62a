# The native caller of the fuse commit (built by __graft_entry__.build() next to the callers of
# Makefile): Planar_SLAM::LocalMapTracker::Fuse / FuseLoop / FuseMatched over stand-in classes whose Replace and AddObservation
# restate MapPoint's and MapLine's, next to the reference's loops on the objects alone.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: fuse_caller

fuse_caller: fuse_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f fuse_caller
