# The native caller of the PnP solver (built by __graft_entry__.build() next to the callers of Makefile): Tracking::Relocalization's
# candidate loop over Planar_SLAM::PnPsolver with the reference's signatures; drfe::PnPBatch fills the tables.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: pnp_caller

pnp_caller: pnp_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f pnp_caller
