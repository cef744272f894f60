# Test infrastructure: the host half of the recruit table (hs_recruit_host.cpp) as a program of its own, no device and no HIP.
# make -f recruit_selftest.mk          -> _build/recruit_selftest (tests/test_cpu_recruit_host.py)
# make -f recruit_selftest.mk asan     -> the same under AddressSanitizer + UBSan (not built by default)
CXX ?= g++
P := ../../hairsplitter_amd/csrc
all: _build/recruit_selftest
_build/recruit_selftest: recruit_selftest.cpp $(P)/hs_recruit_host.cpp $(P)/hs_recruit_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -Wall -o $@ recruit_selftest.cpp $(P)/hs_recruit_host.cpp
asan: _build/recruit_selftest_asan
_build/recruit_selftest_asan: recruit_selftest.cpp $(P)/hs_recruit_host.cpp $(P)/hs_recruit_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -o $@ recruit_selftest.cpp $(P)/hs_recruit_host.cpp
