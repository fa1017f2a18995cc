# The restart tests' drivers (g++ only), beside the ones of Makefile:
#   make -C tests/drivers -f restart.mk
# restart_check over the host bookkeeping source alone (tests/test_restart_host.py), restart_facade
# over the C++ facade, linked against the in-tree libhsddp_amd.so (tests/test_gpu_restart_tick.py).
CXX   ?= g++
FLAGS := -std=c++17 -O2 -Wall -Wextra
PKG   := ../../hkd-mpc_amd
LIB   := -L$(PKG) -lhsddp_amd -Wl,-rpath,'$$ORIGIN/$(PKG)'
HDR   := $(wildcard $(PKG)/facade/*.hpp) ../../include/hsddp.h

all: restart_check restart_facade

restart_check: restart_check.cpp $(PKG)/csrc/hsddp_phases.cpp $(PKG)/csrc/hsddp_phases.h ../../include/hsddp.h
	$(CXX) $(FLAGS) -o $@ restart_check.cpp $(PKG)/csrc/hsddp_phases.cpp

restart_facade: restart_facade.cpp $(HDR) $(PKG)/libhsddp_amd.so
	$(CXX) $(FLAGS) -pthread -I$(PKG)/facade -o $@ restart_facade.cpp $(LIB)

clean:
	rm -f restart_check restart_facade

.PHONY: all clean
