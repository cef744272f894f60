// hs_map_host.h -- the read mapper of include/hairsplitter_hip.h (hs_map_reads): the rule that names, for every read, the contig window it came
// from, stated once for the host and the device. Minimizer seeds and a vote over diagonal bins; no chaining, no base-level alignment (A1 does
// the exact placement inside the window, hs_realign_intervals). The reference has no counterpart (it shells out to minimap2): the rule is ours.
// No device code and no HIP call in here or in hs_map_host.cpp: tests/harness/map_selftest.cpp builds both into a program of its own.
//
// The defaults of hs_map_params are minimap2's ONT k and w plus placeholders (max_occ, band_log2, min_votes). They are NOT tuned.
//
//   k-mer at p       f = forward word (base p most significant, 2 bits a base), r = reverse-complement word (3 - code). Skipped when f == r.
//                    strand bit s = (r < f); hash h = map_mix32(min(f, r)) -- murmur3's 32-bit finaliser, a bijection: equal h = equal k-mer.
//   minimizers       window j = the k-mers j .. j + w - 1; its minimizer = the smallest (h, p) among those not skipped (leftmost on equal h).
//                    A sequence of n >= 1 k-mers has the windows 0 .. max(0, n - w) (fewer than w k-mers: one window of them all). Each
//                    distinct p once, ascending.
//   index            all contig minimizers (h, contig, t, s); occ(h) = entries of h; a read minimizer with occ(h) > max_occ is not looked up.
//   hit              read minimizer (h, q, sq) of a read of Lr bases x entry (h, c, t, st): rel = sq ^ st, qa = rel ? Lr - k - q : q,
//                    d = t - qa, bin = (d + Lr) >> band_log2 (d + Lr >= k). Key = (c, rel, bin), ordered as the 64-bit word of map_key.
//   vote             n(key) = hits of the key; a candidate is a key with n >= 1; score(key) = n(key) + n(key + 1 bin). Best = the largest
//                    score, then the smaller key (smaller c, then rel 0, then the smaller bin): a total order. second = the largest score of a
//                    candidate with another (c, rel) or a bin more than one away from the best's (0: none). Mapped iff best >= min_votes.
//   interval         over the best's hits in its two bins: qa_lo = min qa, qa_hi = max qa + k, t_lo = min t, t_hi = max t + k; with `extend`
//                    stretched to the whole read and clipped at the contig's ends (map_interval).
#ifndef HS_MAP_HOST_H
#define HS_MAP_HOST_H

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/hairsplitter_hip.h"

#include "hs_rules.h"      // HS_HD

namespace hs {

HS_HD inline bool map_params_valid(const hs_map_params& p) {
    return p.k >= 5 && p.k <= 16 && p.w >= 1 && p.w <= 32 && p.max_occ >= 1 && p.band_log2 >= 0 && p.band_log2 <= 30 && p.min_votes >= 1
           && (p.extend == 0 || p.extend == 1) && p.bucket_bits >= -1 && p.bucket_bits <= 26;
}
// bucket_bits = -1: one bucket per contig minimizer, rounded up to a power of two, 2^10 .. 2^26
inline int32_t map_bucket_bits(const hs_map_params& p, int64_t n_entries) {
    if (p.bucket_bits >= 0) return p.bucket_bits;
    int32_t b = 10;
    while (b < 26 && ((int64_t)1 << b) < n_entries) ++b;
    return b;
}

// murmur3's 32-bit finaliser (fmix32): a bijection of the 32-bit words
HS_HD inline uint32_t map_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
HS_HD inline uint32_t map_kmer_mask(int k) { return k >= 16 ? 0xFFFFFFFFu : ((1u << (2 * k)) - 1u); }
// the k-mer that starts at seq[0] (codes 0..3; anything else counts by its low two bits): false = skipped (its own reverse complement)
HS_HD inline bool map_kmer(const uint8_t* seq, int k, uint32_t* h, uint32_t* s) {
    uint32_t f = 0, r = 0;
    for (int i = 0; i < k; ++i) {
        const uint32_t c = seq[i] & 3u;
        f = (f << 2) | c;
        r = (r >> 2) | ((3u - c) << (2 * (k - 1)));
    }
    if (f == r) return false;
    *s = r < f ? 1u : 0u;
    *h = map_mix32(r < f ? r : f);
    return true;
}
// windows of a sequence of n_kmers k-mers (n_kmers >= 1): 0 .. map_last_window
HS_HD inline int64_t map_last_window(int64_t n_kmers, int w) { return n_kmers > w ? n_kmers - w : 0; }

// a hit: its key and its read coordinate on the contig's strand
HS_HD inline uint64_t map_key(int32_t c, uint32_t rel, uint32_t bin) { return ((uint64_t)(uint32_t)c << 33) | ((uint64_t)rel << 32) | bin; }
HS_HD inline int32_t map_key_contig(uint64_t key) { return (int32_t)(key >> 33); }
HS_HD inline uint32_t map_key_rel(uint64_t key) { return (uint32_t)(key >> 32) & 1u; }
HS_HD inline uint64_t map_hit(int32_t c, int32_t t, uint32_t st, int32_t q, uint32_t sq, int32_t Lr, const hs_map_params& p, int32_t* qa) {
    const uint32_t rel = sq ^ st;
    *qa = rel ? Lr - p.k - q : q;
    return map_key(c, rel, (uint32_t)(((int64_t)t - *qa + Lr) >> p.band_log2));
}
// candidate a (score, key) before candidate b?
HS_HD inline bool map_beats(uint32_t sa, uint64_t ka, uint32_t sb, uint64_t kb) { return sa > sb || (sa == sb && ka < kb); }
// may a candidate count for `second` next to the best?
HS_HD inline bool map_second_allowed(uint64_t key, uint64_t best) {
    if ((key >> 32) != (best >> 32)) return true;
    const int64_t d = (int64_t)(uint32_t)key - (int64_t)(uint32_t)best;
    return d > 1 || d < -1;
}
// is a hit with this key one of the best's (its bin or the next)?
HS_HD inline bool map_in_best(uint64_t key, uint64_t best) { return key == best || key == best + 1; }

struct MapVote {
    uint32_t best = 0, second = 0;      // scores; best == 0: no hit at all
    uint64_t key = 0;
    int32_t qa_min = 0, qa_max = 0, t_min = 0, t_max = 0;      // over the best's hits
};
// the per-read record from the vote (Lc = the best contig's length; ignored without a hit)
HS_HD inline void map_interval(const hs_map_params& p, const MapVote& v, int32_t Lr, int32_t Lc, int32_t* contig, uint8_t* strand, int32_t* qstart, int32_t* qend,
                               int32_t* tstart, int32_t* tend) {
    *contig = -1; *strand = 0; *qstart = *qend = *tstart = *tend = 0;
    if (v.best == 0 || v.best < (uint32_t)p.min_votes) return;
    int64_t qa_lo = v.qa_min, qa_hi = (int64_t)v.qa_max + p.k, t_lo = v.t_min, t_hi = (int64_t)v.t_max + p.k;
    if (p.extend) {
        const int64_t tl = t_lo - qa_lo, th = t_hi + (Lr - qa_hi);
        qa_lo = tl < 0 ? -tl : 0; t_lo = tl < 0 ? 0 : tl;
        qa_hi = Lr - (th > Lc ? th - Lc : 0); t_hi = th > Lc ? Lc : th;
    }
    const uint32_t rel = map_key_rel(v.key);
    *contig = map_key_contig(v.key); *strand = (uint8_t)(1 - rel);
    *qstart = (int32_t)(rel ? Lr - qa_hi : qa_lo); *qend = (int32_t)(rel ? Lr - qa_lo : qa_hi);
    *tstart = (int32_t)t_lo; *tend = (int32_t)t_hi;
}

// ---- the device-free half: a whole job on the host ----
struct MapMinimizers {      // (sequence, position) ascending
    std::vector<uint32_t> h, ps;      // ps = position << 1 | strand bit
    std::vector<int32_t> seq;
    std::vector<int64_t> seq_off;      // [n_seqs + 1] into the three
};
void map_minimizers(const uint8_t* seq, const int64_t* off, int32_t n_seqs, const hs_map_params& p, MapMinimizers& out);

struct MapIndexHost {
    hs_map_params params{};
    int32_t n_contigs = 0, bucket_bits = 0;
    std::vector<int64_t> contig_len;
    std::vector<int64_t> bucket_off;      // [2^bucket_bits + 1]
    std::vector<uint32_t> e_h, e_ts;      // entries by bucket; inside a bucket by (h, contig, t)
    std::vector<int32_t> e_c;
};
int map_index_host(const uint8_t* contig_seq, const int64_t* contig_off, int32_t n_contigs, const hs_map_params& p, MapIndexHost& ix, std::string& err);
// per read arrays as hs_map_result has them, sized here; n_threads < 1: one
struct MapResultHost {
    std::vector<int32_t> contig, qstart, qend, tstart, tend, votes, second, n_minimizers, n_skipped;
    std::vector<uint8_t> strand;
    std::vector<int64_t> n_hits;
};
int map_reads_host(const MapIndexHost& ix, const uint8_t* read_seq, const int64_t* read_off, int32_t n_reads, int n_threads, MapResultHost& out, std::string& err);
// PAF lines of the mapped reads: names[] may be nullptr (then r<i> / c<i>)
std::string map_text(const hs_map_result* r, const char* const* read_names, const int64_t* read_len, const char* const* contig_names, const int64_t* contig_len);

}  // namespace hs
#endif
