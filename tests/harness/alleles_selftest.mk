# Test infrastructure: the host half of the allele table (hs_alleles_host.cpp) as a program of its own, no device and no HIP.
# make -f alleles_selftest.mk          -> _build/alleles_selftest (tests/test_cpu_alleles_host.py)
# make -f alleles_selftest.mk asan     -> the same under AddressSanitizer + UBSan (not built by default)
CXX ?= g++
P := ../../hairsplitter_amd/csrc
all: _build/alleles_selftest
_build/alleles_selftest: alleles_selftest.cpp $(P)/hs_alleles_host.cpp $(P)/hs_alleles_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -Wall -o $@ alleles_selftest.cpp $(P)/hs_alleles_host.cpp
asan: _build/alleles_selftest_asan
_build/alleles_selftest_asan: alleles_selftest.cpp $(P)/hs_alleles_host.cpp $(P)/hs_alleles_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -o $@ alleles_selftest.cpp $(P)/hs_alleles_host.cpp
