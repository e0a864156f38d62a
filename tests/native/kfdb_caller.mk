# The native caller of KeyFrameDatabase (built by __graft_entry__.build() next to the callers of Makefile):
# Planar_SLAM::KeyFrameDatabase with the reference's five signatures and its two batch forms over stand-in key frames and frames.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/dr_slam_amd/csrc
CFLAGS := -O2 -Wall -Wextra -I$(ROOT)/include
LDFLAGS := -L$(LIBDIR) -ldrfe -Wl,-rpath,'$$ORIGIN/../../dr_slam_amd/csrc' -Wl,-rpath,/opt/rocm/lib

all: kfdb_caller

kfdb_caller: kfdb_caller.cpp $(ROOT)/include/drfe_adaptor.hpp $(ROOT)/include/drfe.h
	g++ -std=c++17 $(CFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f kfdb_caller
