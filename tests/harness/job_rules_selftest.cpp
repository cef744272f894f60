// TEST INFRASTRUCTURE: what hs_job_rules.h -- the very functions the drivers, the pipeline calls and the executables call -- gives,
// printed for tests/test_cpu_rules.py to hold against the Python forms of hairsplitter_amd/dist.py. Built with -ffp-contract=off
// like the product. stdin, one case per line:
//   "er <n> <n float bit patterns as hex>"  -> "er <bits of hs::job_error_rate> <number of positive entries> <bits of
//                                               hs::error_rate_as_stage4_reads_it of it>"
//   "ws <sum> <n_reads> <above_4000>"       -> "ws <hs::window_size_from_counts>" (sum: unsigned 64-bit, wrapped to 32 bits here
//                                               as a caller's running uint32_t sum would have)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../hairsplitter_amd/csrc/hs_job_rules.h"
static uint32_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
int main() {
    char kind[8];
    while (std::scanf("%7s", kind) == 1) {
        if (!std::strcmp(kind, "er")) {
            int n = 0;
            if (std::scanf("%d", &n) != 1 || n < 0) return 2;
            std::vector<float> v((size_t)n);
            for (int i = 0; i < n; ++i) { unsigned b; if (std::scanf("%x", &b) != 1) return 2; const uint32_t u = b; std::memcpy(&v[(size_t)i], &u, 4); }
            int pos = -1;
            const float er = hs::job_error_rate(v.data(), n, &pos);
            std::printf("er %08x %d %08x\n", bits_of(er), pos, bits_of(hs::error_rate_as_stage4_reads_it(er)));
        } else if (!std::strcmp(kind, "ws")) {
            unsigned long long sum; long long n, above;
            if (std::scanf("%llu %lld %lld", &sum, &n, &above) != 3) return 2;
            std::printf("ws %d\n", (int)hs::window_size_from_counts((uint32_t)sum, n, above));
        } else return 2;
    }
    return 0;
}
