# Test infrastructure: the device-free additions of the haplotype route (the FASTA record, the plan of a piece) as a program of its own, no device and no HIP.
# make -f haplotypes_selftest.mk          -> _build/haplotypes_selftest (tests/test_cpu_haplotypes.py)
# make -f haplotypes_selftest.mk asan     -> the same under AddressSanitizer + UBSan, an executable of its own (tests/test_cpu_haplotypes.py runs it once)
CXX ?= g++
P := ../../hairsplitter_amd/csrc
all: _build/haplotypes_selftest
_build/haplotypes_selftest: haplotypes_selftest.cpp $(P)/hs_haplotypes_host.h $(P)/hs_consensus_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -Wall -o $@ haplotypes_selftest.cpp
asan: _build/haplotypes_selftest_asan
_build/haplotypes_selftest_asan: haplotypes_selftest.cpp $(P)/hs_haplotypes_host.h $(P)/hs_consensus_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -o $@ haplotypes_selftest.cpp
