# The native caller of LocalMapping::ProcessNewKeyFrame's item loops (built by __graft_entry__.build() next to the callers of
# Makefile): Planar_SLAM::LocalMapTracker::ProcessNewKeyFrame over stand-in classes whose AddObservation restates MapPoint's and
# MapLine's, next to the reference's loop (src/LocalMapping.cc:124-157) with UpdateNormalAndDepth on the objects alone.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: insert_caller

insert_caller: insert_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f insert_caller
