# The terrain tests' drivers (g++ only), beside the ones of Makefile, restart.mk and elements.mk:
#   make -C tests/drivers -f terrain.mk
# terrain_check over the host bookkeeping source alone (tests/test_terrain_host.py), terrain_facade
# over the C++ facade, linked against the in-tree libhsddp_amd.so (tests/test_terrain_host.py: its
# host mode; tests/test_gpu_terrain.py: its device mode).
CXX   ?= g++
FLAGS := -std=c++17 -O2 -Wall -Wextra
PKG   := ../../hkd-mpc_amd
LIB   := -L$(PKG) -lhsddp_amd -Wl,-rpath,'$$ORIGIN/$(PKG)'
HDR   := $(wildcard $(PKG)/facade/*.hpp) ../../include/hsddp.h

all: terrain_check terrain_facade

terrain_facade: terrain_facade.cpp $(HDR) $(PKG)/libhsddp_amd.so
	$(CXX) $(FLAGS) -I$(PKG)/facade -o $@ terrain_facade.cpp $(LIB)

terrain_check: terrain_check.cpp $(PKG)/csrc/hsddp_phases.cpp $(PKG)/csrc/hsddp_phases.h ../../include/hsddp.h
	$(CXX) $(FLAGS) -o $@ terrain_check.cpp $(PKG)/csrc/hsddp_phases.cpp

clean:
	rm -f terrain_check terrain_facade

.PHONY: all clean
