# The native caller of LocalMapping::KeyFrameCulling (built by __graft_entry__.build() next to the callers of Makefile):
# Planar_SLAM::LocalMapTracker::SyncCulling / KeyFrameCulling over stand-in classes whose SetBadFlag and EraseObservation restate
# src/KeyFrame.cc:574-705 and src/MapPoint.cc:145-202.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: cull_caller

cull_caller: cull_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f cull_caller
