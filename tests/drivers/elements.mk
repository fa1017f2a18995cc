# The element-move test's driver (g++ only), beside the ones of Makefile and restart.mk:
#   make -C tests/drivers -f elements.mk
# elements_check over the host bookkeeping source alone (tests/test_elements_host.py).
CXX   ?= g++
FLAGS := -std=c++17 -O2 -Wall -Wextra
PKG   := ../../hkd-mpc_amd

all: elements_check

elements_check: elements_check.cpp $(PKG)/csrc/hsddp_phases.cpp $(PKG)/csrc/hsddp_phases.h ../../include/hsddp.h
	$(CXX) $(FLAGS) -o $@ elements_check.cpp $(PKG)/csrc/hsddp_phases.cpp

clean:
	rm -f elements_check

.PHONY: all clean
