// TEST INFRASTRUCTURE: what hs_rules.h -- the very functions the kernels and the host code call -- gives, printed for
// tests/test_cpu_rules.py to hold against the independent restatements (tests/chi_tables.py, the numpy predicate of
// tests/test_gpu_kernels.py, the hash-map emulator of hs_rh8.h). Built with -ffp-contract=off like the product.
//   stdin: one 2x2 table "n00 n01 n10 n11" per line   -> "chi <bits of hs::chi_square as hex>" per table
//   then, for all code pairs 33..157 x 33..157        -> 125 lines "cbt <125 x 0/1>" (row k0, column k1)
//   then, for all 256 keys and both widths            -> "rank <key> <wide> <hs::rh8_static_rank> <home bucket> <info byte>", the last two
//                                                         from Rh8::home of a fresh map of 8 / 16 buckets
#include <cstdio>
#include <cstring>
#include "../../hairsplitter_amd/csrc/hs_rh8.h"
#include "../../hairsplitter_amd/csrc/hs_rules.h"
int main() {
    int t[4];
    while (std::scanf("%d %d %d %d", &t[0], &t[1], &t[2], &t[3]) == 4) {
        const float chi = hs::chi_square(t[0], t[1], t[2], t[3]);
        uint32_t bits;
        std::memcpy(&bits, &chi, 4);
        std::printf("chi %08x\n", bits);
    }
    for (int k0 = 33; k0 <= 157; ++k0) {
        std::printf("cbt ");
        for (int k1 = 33; k1 <= 157; ++k1) std::putchar(hs::central_base_test(k0, k1) ? '1' : '0');
        std::putchar('\n');
    }
    for (int wide = 0; wide < 2; ++wide)
        for (int k = 0; k < 256; ++k) {
            hs::Rh8 rh; rh.clear();
            rh.alloc(wide ? 16 : 8);
            if (wide) rh.mult += hs::kRh8MultStep;      // (the map has grown once: robin_hood.h:2448)
            int idx; uint32_t inf;
            rh.home((uint8_t)k, idx, inf);
            std::printf("rank %d %d %d %d %u\n", k, wide, hs::rh8_static_rank(k, wide != 0), idx, inf);
        }
    return 0;
}
