# The native caller of LocalMapping::MapPlaneCulling (built by __graft_entry__.build() next to the callers of Makefile):
# drfe::MapPlaneCulling over stand-in MapPlane / KeyFrame classes next to the reference's walk written against the same classes.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: plane_cull_caller

plane_cull_caller: plane_cull_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f plane_cull_caller
