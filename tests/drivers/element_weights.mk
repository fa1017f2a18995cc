# The per-robot weights tests' driver (g++ only), beside the ones of Makefile and terrain.mk:
#   make -C tests/drivers -f element_weights.mk
# element_weights_check over the dispatch header and the host bookkeeping source alone
# (tests/test_element_weights_host.py).
CXX   ?= g++
FLAGS := -std=c++17 -O2 -Wall -Wextra
PKG   := ../../hkd-mpc_amd

all: element_weights_check

element_weights_check: element_weights_check.cpp $(PKG)/csrc/hsddp_dispatch.h $(PKG)/csrc/hsddp_phases.cpp $(PKG)/csrc/hsddp_phases.h ../../include/hsddp.h
	$(CXX) $(FLAGS) -I$(PKG)/csrc -o $@ element_weights_check.cpp $(PKG)/csrc/hsddp_phases.cpp

clean:
	rm -f element_weights_check

.PHONY: all clean
