// TEST INFRASTRUCTURE: the rule the kernels use (hs::rh8_static_rank of hs_rules.h: K4's column_vs_partition_dev, K3b's
// k_column_top3_exact, loop A's k_loop_a_prepare) to break ties between second alleles without replaying the insertions on the
// hash-map emulator -- "a robin_hood map of up to 12 char keys iterates them by (home bucket ascending, low
// five hash bits descending, insertion order), 8 buckets up to 6 keys, 16 buckets and the next multiplier from 7 to 12, unless
// some key sits 6 or more slots from its home bucket" -- against hs_rh8.h (itself pinned to the reference's header by
// tests/golden/robin_hood_order.json) on random key sets, half of them from small alphabets so that buckets collide.
// Prints "checked <n> bad <m> ..."; exit code 1 if any pair of keys with different ranks comes out in another order.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../hairsplitter_amd/csrc/hs_rh8.h"
#include "../../hairsplitter_amd/csrc/hs_rules.h"
int main(int argc, char** argv) {
    const long trials = argc > 1 ? std::atol(argv[1]) : 2000000;
    long bad = 0, checked = 0, collisions = 0, displaced = 0;
    srand(3);
    for (long it = 0; it < trials; ++it) {
        int n = 1 + rand() % 12;
        const int alpha = (it & 1) ? 125 : 24;
        if (n > alpha) n = alpha;
        std::vector<uint8_t> keys;
        const int base = 33 + rand() % (126 - alpha);
        while ((int)keys.size() < n) { const uint8_t k = (uint8_t)(base + rand() % alpha); if (std::find(keys.begin(), keys.end(), k) == keys.end()) keys.push_back(k); }
        hs::Rh8 rh; rh.clear();
        for (uint8_t k : keys) rh.insert(k);
        uint8_t ord[300]; const int m = rh.order(ord);
        const bool big = n > 6;
        std::vector<int> rank((size_t)n);
        int cnt[16] = {0};
        for (int i = 0; i < n; ++i) { rank[(size_t)i] = hs::rh8_static_rank(keys[(size_t)i], big); cnt[rank[(size_t)i] >> 5]++; }
        bool far = false;
        if (big) { int carry = 0; for (int b = 0; b < 16; ++b) { if (cnt[b] > 0 && carry + cnt[b] - 1 >= 6) far = true; carry = std::max(0, carry + cnt[b] - 1); } }
        if (far) { displaced++; continue; }      // the kernel hands these to the emulator
        int where[256];
        for (int i = 0; i < m; ++i) where[ord[i]] = i;
        bool dup = false;
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
            if (i != j && rank[(size_t)i] == rank[(size_t)j]) dup = true;
            if (rank[(size_t)i] < rank[(size_t)j] && where[keys[(size_t)i]] > where[keys[(size_t)j]]) bad++;
        }
        if (m != n) bad++;
        collisions += dup; checked++;
    }
    std::printf("checked %ld bad %ld sets-with-equal-ranks %ld sets-with-a-far-key %ld\n", checked, bad, collisions, displaced);
    return bad ? 1 : 0;
}
