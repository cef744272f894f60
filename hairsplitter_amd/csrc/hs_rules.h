// hs_rules.h -- the small rules of the reference that the column tests rest on, each stated ONCE for the host code, the
// kernels and the test harness (plain C++, no HIP headers: g++ compiles it for the host and the harness, hipcc for the
// device). Citations are call_variants.cpp of the reference unless another file is named. Every translation unit that
// includes it is built with -ffp-contract=off (and the device code with IEEE division), so the float results are the same
// bits everywhere. Pinned by tests/test_cpu_rules.py (tests/harness/rules_selftest.cpp) and tests/harness/rh8_static_order.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HS_HD __host__ __device__
#else
#define HS_HD
#endif
// the small rules are always inlined: the kernels get the code they had when each of them spelled the rule out
#define HS_RULE HS_HD inline __attribute__((always_inline))

namespace hs {

// computeChiSquare (:1135-1163) on the 2x2 table n<state +1 ? 1 : 0><reference allele ? 1 : 0> (second allele / state -1: 0):
// float marginals, double squares, float result; 0 for an empty table or one degenerate margin, -1 for two
HS_RULE float chi_square(int n00, int n01, int n10, int n11) {
    const int n = n00 + n01 + n10 + n11;
    if (n == 0) return 0;
    const float pmax1 = float(n10 + n11) / n;
    const float pmax2 = float(n01 + n11) / n;
    if (pmax1 * (1 - pmax1) == 0 && pmax2 * (1 - pmax2) == 0) return -1;
    if (pmax1 * pmax2 * (1 - pmax1) * (1 - pmax2) == 0) return 0;
    const float e00 = (1 - pmax1) * (1 - pmax2) * n, e01 = (1 - pmax1) * pmax2 * n;
    const float e10 = pmax1 * (1 - pmax2) * n, e11 = pmax1 * pmax2 * n;
    const double d00 = (double)(float)(n00 - e00), d01 = (double)(float)(n01 - e01);
    const double d10 = (double)(float)(n10 - e10), d11 = (double)(float)(n11 - e11);
    return (float)(d00 * d00 / (double)e00 + d01 * d01 / (double)e01 + d10 * d10 / (double)e10 + d11 * d11 / (double)e11);
}

// the verdict of loops C (:721-738) and D (:745-764) of keep_only_robust_variants on one table, `chi` its chi_square and `n`
// the column's depth: loop C keeps a candidate column, loop D rescues one that passes central_base_test with a second count >= 5
HS_RULE bool loop_cd_keeps(int n00, int n01, int n10, int n11, float chi, int n, bool loop_c, bool loop_d) {
    return (loop_c && (double)(n00 + n01 + n10 + n11) > 0.5 * (double)n && chi > 15) ||
           (loop_d && (double)chi > 20.0 && n10 + n00 > 4 && n01 + n11 > 4);
}

// :527-528 and :751-752 (the same predicate on the raw bytes of the two leading pileup codes)
HS_RULE bool central_base_test(int k0, int k1) {
    return k0 % 5 != k1 % 5 && ((k1 - '!') % 5 != 4 || (k1 / 5 % 5 != k0 % 5 && k1 / 25 % 5 != k0 % 5));
}

// robin_hood.h 3.11.1: the murmur step of hash_int (:749-760) followed by the map's own multiplier (keyToIdx :1349-1361). The low five bits
// of the result make the info byte, the bits above them the home bucket. A map starts with kRh8Mult and adds kRh8MultStep
// every time it grows or rehashes (:2413-2443).
constexpr uint64_t kRh8Mult = 0xc4ceb9fe1a85ec53ull;
constexpr uint64_t kRh8MultStep = 0xc4ceb9fe1a85ec54ull;
HS_RULE uint64_t rh8_mix(uint8_t key, uint64_t mult) {
    uint64_t h = (uint64_t)key;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
    h *= mult; h ^= h >> 33;
    return h;
}

// place of a byte key in the iteration order of robin_hood::unordered_flat_map<unsigned char, int> while it holds at most 12
// keys: up to 6 keys 8 buckets and the first multiplier, 7 to 12 keys (`wide`) 16 buckets and the second one;
// rank = home bucket << 5 | 31 - low five hash bits. Keys of different rank iterate in rank order whatever order they were
// inserted in, unless (wide only) a key sits six or more slots from its bucket; keys of equal rank and such sets go through
// the emulator of hs_rh8.h. Checked against the emulator on 2 M key sets by tests/harness/rh8_static_order.cpp.
HS_RULE int rh8_static_rank(int key, bool wide) {
    const uint64_t h = rh8_mix((uint8_t)key, wide ? kRh8Mult + kRh8MultStep : kRh8Mult);
    return (int)((((h >> 5) & (wide ? 15ull : 7ull)) << 5) | (31ull - (h & 31ull)));
}

// The second allele: the most frequent eligible code among `seen` (distinct codes in first-appearance order, cnt[i] reads
// each), the first in the hash map's iteration order among equal counts (:837-844, Partition.cpp:59-66). `signed_ref_quirk`:
// in distance() the reference compares a *signed* char with unsigned keys (:838), so a reference code >= 128 never equals a
// key and stays eligible; `insert_ref_last`: content2[ref] then inserts it as a zero-count key. `rh` is an empty hs::Rh8 or
// hs::Rh8View and `ord` room for its keys (255 at most; the device keeps both in LDS): touched on a tie only.
template <class Map, class Code, class Count>
HS_HD int second_from_seen(Map& rh, uint8_t* ord, const Code* seen, const Count* cnt, int nseen, int ref, bool signed_ref_quirk,
                                  bool insert_ref_last, int dflt) {
    if (nseen == 0) return dflt;
    const bool ref_eligible = signed_ref_quirk && ref >= 128;
    int best = -1, nbest = 0, bestk = dflt;
    bool ref_seen = false;
    for (int i = 0; i < nseen; ++i) {
        const int k = (int)seen[i];
        if (k == ref) { ref_seen = true; if (!ref_eligible) continue; }
        if ((int)cnt[i] > best) { best = (int)cnt[i]; nbest = 1; bestk = k; } else if ((int)cnt[i] == best) nbest++;
    }
    if (ref_eligible && !ref_seen && insert_ref_last) { if (0 > best) { best = 0; nbest = 1; bestk = ref; } else if (best == 0) nbest++; }
    if (best < 0) return dflt;
    if (nbest == 1) return bestk;
    for (int i = 0; i < nseen; ++i) rh.insert((uint8_t)seen[i]);
    if (insert_ref_last) rh.insert((uint8_t)ref);
    const int m = rh.order(ord);
    for (int i = 0; i < m; ++i) {
        const int k = ord[i];
        if (k == ref && !ref_eligible) continue;
        int c = 0;
        for (int j = 0; j < nseen; ++j) if ((int)seen[j] == k) { c = (int)cnt[j]; break; }
        if (c == best) return k;
    }
    return bestk;
}

}  // namespace hs
