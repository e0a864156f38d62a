# The native caller of what surrounds the solver of Optimizer::OptimizeEssentialGraph (built by __graft_entry__.build() next to the callers of Makefile):
# Planar_SLAM::LocalMapTracker::EssentialEdges / EssentialCommit over stand-in classes next to a pointer-walking restatement of src/Optimizer.cc:2910-3131.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: essential_caller

essential_caller: essential_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f essential_caller
