# The native caller of TranslationOptimization (built by __graft_entry__.build() next to the callers of Makefile):
# Planar_SLAM::Optimizer::TranslationOptimization with the reference's signature and drfe::TransOptBatch over stand-in frames.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: trans_opt_caller

trans_opt_caller: trans_opt_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f trans_opt_caller
