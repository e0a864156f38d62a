# The native caller of the Sim3 solver (built by __graft_entry__.build() next to the callers of Makefile): LoopClosing::ComputeSim3's
# candidate loop over Planar_SLAM::Sim3Solver with the reference's signatures; drfe::Sim3Batch fills the tables.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: sim3_caller

sim3_caller: sim3_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f sim3_caller
