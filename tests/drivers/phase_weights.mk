# The per-phase weights tests' drivers (g++ only), beside the ones of Makefile, restart.mk, elements.mk,
# terrain.mk and element_weights.mk:
#   make -C tests/drivers -f phase_weights.mk
# phase_weights_check over the host bookkeeping source alone (tests/test_phase_weights_host.py), built a
# second time with the address and undefined-behaviour sanitizers as the stand-alone program it is;
# phase_weights_facade over the C++ facade, linked against the in-tree libhsddp_amd.so
# (tests/test_phase_weights_host.py: its host mode; tests/test_gpu_phase_weights.py: its device mode).
CXX   ?= g++
FLAGS := -std=c++17 -O2 -Wall -Wextra
PKG   := ../../hkd-mpc_amd
SRC   := phase_weights_check.cpp $(PKG)/csrc/hsddp_phases.cpp
DEP   := $(SRC) $(PKG)/csrc/hsddp_phases.h ../../include/hsddp.h
LIB   := -L$(PKG) -lhsddp_amd -Wl,-rpath,'$$ORIGIN/$(PKG)'
HDR   := $(wildcard $(PKG)/facade/*.hpp) ../../include/hsddp.h

all: phase_weights_check phase_weights_check_san phase_weights_facade

phase_weights_facade: phase_weights_facade.cpp $(HDR) $(PKG)/libhsddp_amd.so
	$(CXX) $(FLAGS) -I$(PKG)/facade -o $@ phase_weights_facade.cpp $(LIB)

phase_weights_check: $(DEP)
	$(CXX) $(FLAGS) -o $@ $(SRC)

phase_weights_check_san: $(DEP)
	$(CXX) $(FLAGS) -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ $(SRC)

clean:
	rm -f phase_weights_check phase_weights_check_san phase_weights_facade

.PHONY: all clean
