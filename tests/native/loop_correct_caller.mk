# The native caller of LoopClosing::CorrectLoop's Sim3 propagation (built by __graft_entry__.build() next to the callers of Makefile):
# Planar_SLAM::LocalMapTracker::CorrectLoop over stand-in classes next to a pointer-walking restatement of src/LoopClosing.cc:480-562.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: loop_correct_caller

loop_correct_caller: loop_correct_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f loop_correct_caller
