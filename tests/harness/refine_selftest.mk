# Test infrastructure: the device-free half of the polishing passes (hs_refine_host.cpp on hs_consensus_host.cpp) as a program of its own, no device and no HIP.
# make -f refine_selftest.mk          -> _build/refine_selftest (tests/test_cpu_refine.py)
# make -f refine_selftest.mk asan     -> the same under AddressSanitizer + UBSan, an executable of its own (tests/test_cpu_refine.py runs it once)
CXX ?= g++
P := ../../hairsplitter_amd/csrc
SRC := refine_selftest.cpp $(P)/hs_refine_host.cpp $(P)/hs_consensus_host.cpp
DEP := $(SRC) $(P)/hs_refine_host.h $(P)/hs_consensus_host.h $(P)/hs_rules.h
all: _build/refine_selftest
_build/refine_selftest: $(DEP)
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -Wall -o $@ $(SRC) -lpthread
asan: _build/refine_selftest_asan
_build/refine_selftest_asan: $(DEP)
	@mkdir -p _build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -o $@ $(SRC) -lpthread
