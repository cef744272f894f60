# Test infrastructure: the device-free half of the bundle consensus (hs_consensus_host.cpp) as a program of its own, no device and no HIP.
# make -f consensus_selftest.mk          -> _build/consensus_selftest (tests/test_cpu_consensus.py)
# make -f consensus_selftest.mk asan     -> the same under AddressSanitizer + UBSan, an executable of its own (tests/test_cpu_consensus.py runs it once)
CXX ?= g++
P := ../../hairsplitter_amd/csrc
all: _build/consensus_selftest
_build/consensus_selftest: consensus_selftest.cpp $(P)/hs_consensus_host.cpp $(P)/hs_consensus_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -Wall -o $@ consensus_selftest.cpp $(P)/hs_consensus_host.cpp -lpthread
asan: _build/consensus_selftest_asan
_build/consensus_selftest_asan: consensus_selftest.cpp $(P)/hs_consensus_host.cpp $(P)/hs_consensus_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -o $@ consensus_selftest.cpp $(P)/hs_consensus_host.cpp -lpthread
