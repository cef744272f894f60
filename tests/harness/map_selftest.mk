# Test infrastructure: the device-free half of the read mapper (hs_map_host.cpp) as a program of its own, no device and no HIP.
# make -f map_selftest.mk          -> _build/map_selftest (tests/test_cpu_map_cases.py, tests/test_gpu_map.py)
# make -f map_selftest.mk asan     -> the same under AddressSanitizer + UBSan, an executable of its own (tests/test_cpu_map_cases.py runs it once)
CXX ?= g++
P := ../../hairsplitter_amd/csrc
all: _build/map_selftest
_build/map_selftest: map_selftest.cpp map_job_io.h $(P)/hs_map_host.cpp $(P)/hs_map_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -Wall -o $@ map_selftest.cpp $(P)/hs_map_host.cpp -lpthread
asan: _build/map_selftest_asan
_build/map_selftest_asan: map_selftest.cpp map_job_io.h $(P)/hs_map_host.cpp $(P)/hs_map_host.h $(P)/hs_rules.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -o $@ map_selftest.cpp $(P)/hs_map_host.cpp -lpthread
