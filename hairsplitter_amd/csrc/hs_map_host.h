// hs_map_host.h -- the read mapper of include/hairsplitter_hip.h (hs_map_reads): the rule that names, for every read, the contig window it came
// from, stated once for the host and the device. Minimizer seeds and a vote over diagonal bins; no chaining, no base-level alignment (A1 does
// the exact placement inside the window, hs_realign_intervals). The reference has no counterpart (it shells out to minimap2): the rule is ours.
// hs_map_reads names one window per read; hs_map_reads_split (below, "split mappings") up to max_segments over disjoint stretches of the read.
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
// seeds [qa_lo, qa_hi) x [t_lo, t_hi) on the contig's strand, stretched along their diagonal to the read range [b0, b1) (the same strand) and
// clipped at the contig's ends; then turned to the read as given. The one statement of `extend` for map_interval and map_segment_interval.
HS_HD inline void map_stretch(const hs_map_params& p, uint32_t rel, int64_t qa_lo, int64_t qa_hi, int64_t t_lo, int64_t t_hi, int32_t Lr, int32_t Lc, int64_t b0, int64_t b1,
                              int32_t* qstart, int32_t* qend, int32_t* tstart, int32_t* tend) {
    if (p.extend) {
        const int64_t tl = t_lo - (qa_lo - b0), th = t_hi + (b1 - qa_hi);
        qa_lo = b0 + (tl < 0 ? -tl : 0); t_lo = tl < 0 ? 0 : tl;
        qa_hi = b1 - (th > Lc ? th - Lc : 0); t_hi = th > Lc ? Lc : th;
    }
    *qstart = (int32_t)(rel ? Lr - qa_hi : qa_lo); *qend = (int32_t)(rel ? Lr - qa_lo : qa_hi);
    *tstart = (int32_t)t_lo; *tend = (int32_t)t_hi;
}
// the per-read record from the vote (Lc = the best contig's length; ignored without a hit)
HS_HD inline void map_interval(const hs_map_params& p, const MapVote& v, int32_t Lr, int32_t Lc, int32_t* contig, uint8_t* strand, int32_t* qstart, int32_t* qend,
                               int32_t* tstart, int32_t* tend) {
    *contig = -1; *strand = 0; *qstart = *qend = *tstart = *tend = 0;
    if (v.best == 0 || v.best < (uint32_t)p.min_votes) return;
    const uint32_t rel = map_key_rel(v.key);
    *contig = map_key_contig(v.key); *strand = (uint8_t)(1 - rel);
    map_stretch(p, rel, v.qa_min, (int64_t)v.qa_max + p.k, v.t_min, (int64_t)v.t_max + p.k, Lr, Lc, 0, Lr, qstart, qend, tstart, tend);
}

// ---- split mappings (hs_map_reads_split): up to max_segments intervals over disjoint stretches of a read ----
// The defaults of hs_map_split_params (4, 3, 100, 200) are placeholders like the mapper's own. They are NOT tuned.
//
//   q                a hit's k-mer starts at q = rel ? Lr - k - qa : qa on the read as given (map_hit_q): nothing new is stored per hit.
//   rounds           0 .. max_segments - 1; `spans` = the seed spans [a0, a1) of the segments taken so far, read as given, in the order taken.
//   free             a hit whose k-mer overlaps no span: q + k <= a0 || q >= a1 for every span (map_hit_free). Round 0: every hit.
//   vote             the vote above over the free hits only; the threshold is the index's min_votes in round 0 and the split min_votes later
//                    (map_round_threshold). No free hit, or a best below the threshold: the read's rounds END (no other candidate is tried).
//   gap              the spans are disjoint, and a free k-mer lies wholly inside one maximal stretch of [0, Lr) outside them: gap g = the number
//                    of spans that end at or before q (map_hit_gap; 0 = leftmost; a gap between two spans that touch is empty and holds no hit).
//                    Of the best's free hits (its bin and the next) the gap with the most is kept, the leftmost on a tie (map_best_gap); the
//                    segment's hits are the best's in that gap, n their number; the best's hits in other gaps stay free.
//   segment          extremes over its hits as above. Rounds >= 1: n < min_votes or qa_hi - qa_lo < min_span ENDS the rounds (map_segment_stands).
//                    Seed span = [qa_lo, qa_hi), or [Lr - qa_hi, Lr - qa_lo) for rel 1 (map_seed_span). Recorded: round, key, n, and `second` as
//                    the vote gives it in round 0, 0 in later rounds.
//   intervals        segments by span start (map_segments_sort). Segment i may use the read range [A0, A1): A0 = the previous span's end (0 for
//                    the first), A1 = the next span's start (Lr for the last) -- but an inner side whose distance to the neighbour's span is
//                    above max_gap stays at the segment's own span bound (map_segment_range): a wide gap is a foreign insert and is left
//                    unaligned, a narrow one a breakpoint both neighbours may cover. With `extend` the seeds are stretched to [A0, A1) and
//                    clipped at the contig's ends (map_stretch); without, the interval is the seed extremes. One segment = map_interval's record.
//   decided here     a segment's `votes` is n (round 0: the vote's best score, since round 0 has one gap). The per-read votes / second of
//                    hs_map_segments are round 0's vote, also for a read without a segment, as hs_map_result has them.
#define HS_MAP_MAX_SEGMENTS 8
HS_HD inline bool map_split_params_valid(const hs_map_split_params& s) {
    return s.max_segments >= 1 && s.max_segments <= HS_MAP_MAX_SEGMENTS && s.min_votes >= 1 && s.min_span >= 0 && s.max_gap >= 0;
}
HS_HD inline int32_t map_hit_q(int32_t qa, uint32_t rel, int32_t Lr, int k) { return rel ? Lr - k - qa : qa; }
HS_HD inline bool map_hit_free(const int32_t* a0, const int32_t* a1, int n_spans, int32_t q, int k) {
    for (int i = 0; i < n_spans; ++i)
        if (!(q + k <= a0[i] || q >= a1[i])) return false;
    return true;
}
HS_HD inline int map_hit_gap(const int32_t* a1, int n_spans, int32_t q) {
    int g = 0;
    for (int i = 0; i < n_spans; ++i) g += a1[i] <= q ? 1 : 0;
    return g;
}
HS_HD inline int map_best_gap(const uint32_t* cnt, int n_gaps) {
    int g = 0;
    for (int i = 1; i < n_gaps; ++i) if (cnt[i] > cnt[g]) g = i;
    return g;
}
HS_HD inline uint32_t map_round_threshold(const hs_map_params& p, const hs_map_split_params& s, int round) { return (uint32_t)(round == 0 ? p.min_votes : s.min_votes); }
HS_HD inline bool map_segment_stands(const hs_map_split_params& s, int round, uint32_t n, int64_t qa_lo, int64_t qa_hi) {
    return round == 0 || (n >= (uint32_t)s.min_votes && qa_hi - qa_lo >= s.min_span);
}
HS_HD inline void map_seed_span(uint32_t rel, int32_t Lr, int64_t qa_lo, int64_t qa_hi, int32_t* a0, int32_t* a1) {
    *a0 = (int32_t)(rel ? Lr - qa_hi : qa_lo); *a1 = (int32_t)(rel ? Lr - qa_lo : qa_hi);
}
struct MapSegment {      // (no initialisers: the kernels keep a read's segments in LDS)
    uint64_t key;
    uint32_t n, second;
    int32_t round, qa_min, qa_max, t_min, t_max, a0, a1;      // [a0, a1): the seed span on the read as given
};
// (spans are disjoint: their starts are distinct)
HS_HD inline void map_segments_sort(MapSegment* s, int n) {
    for (int i = 1; i < n; ++i) {
        const MapSegment x = s[i];
        int j = i;
        for (; j > 0 && s[j - 1].a0 > x.a0; --j) s[j] = s[j - 1];
        s[j] = x;
    }
}
HS_HD inline void map_segment_range(const MapSegment* s, int n, int i, int32_t Lr, int32_t max_gap, int32_t* A0, int32_t* A1) {
    *A0 = i > 0 ? s[i - 1].a1 : 0;
    *A1 = i + 1 < n ? s[i + 1].a0 : Lr;
    if (i > 0 && s[i].a0 - s[i - 1].a1 > max_gap) *A0 = s[i].a0;
    if (i + 1 < n && s[i + 1].a0 - s[i].a1 > max_gap) *A1 = s[i].a1;
}
// the record of segment i of a read's sorted segments (Lc = its contig's length)
HS_HD inline void map_segment_interval(const hs_map_params& p, const hs_map_split_params& sp, const MapSegment* s, int n, int i, int32_t Lr, int32_t Lc, int32_t* contig, uint8_t* strand,
                                       int32_t* qstart, int32_t* qend, int32_t* tstart, int32_t* tend) {
    int32_t A0, A1;
    map_segment_range(s, n, i, Lr, sp.max_gap, &A0, &A1);
    const uint32_t rel = map_key_rel(s[i].key);
    *contig = map_key_contig(s[i].key); *strand = (uint8_t)(1 - rel);
    map_stretch(p, rel, s[i].qa_min, (int64_t)s[i].qa_max + p.k, s[i].t_min, (int64_t)s[i].t_max + p.k, Lr, Lc, rel ? Lr - A1 : A0, rel ? Lr - A0 : A1, qstart, qend, tstart, tend);
}

// ---- anchors (hs_map_reads_anchored): cut points of a mapped read along the chain of its best candidate's hits ----
// The default of hs_map_anchor_params (spacing 256) was a placeholder like the mapper's own and is the fastest of one sweep on one job.
// It is NOT tuned beyond that.
//
//   hits             the read's hits that are the best's (map_in_best), as pairs (qa, t): qa on the read as it aligns (the hits' own coordinate), t on
//                    the contig. Repeats give duplicates in qa or in t.
//   chain            the longest subsequence strictly increasing in qa and in t; of several, the one map_anchor_chain gives: the hits ordered by
//                    (qa ascending, t descending) -- ascending map_anchor_key --, patience over t with a lower-bound search (the first tail >= t is
//                    replaced, or the tails grow by one), a hit's predecessor = the tail of the next shorter length when the hit was placed, the
//                    chain read back from the final tail of the greatest length. Ordered hits already strictly increasing in t: all of them.
//   support          a chain member is supported when its diagonal t - qa equals that of the member before it or after it (map_anchor_supported):
//                    a seed alone on its diagonal between two indel-free runs is not trusted as a cut.
//   cut points       over the supported members in order: the first; then each whose qa is at least `spacing` above the LAST CUT POINT's qa
//                    (map_anchor_cuts). At most Lr / spacing + 1 of them (map_anchor_bound).
//   no anchors       an unmapped read; a read with more hits than hs_map_lds_capacity() (the wide route; n_wide counts those), which is aligned
//                    the plain way. n_best, n_chain and n_supported of such a read are 0.
#define HS_MAP_ANCHOR_NONE 0xFFFFu
#define HS_MAP_ANCHOR_CAPACITY 4096      /* == hs_map_lds_capacity(): hits of a read beyond which it has no anchors */
HS_HD inline bool map_anchor_params_valid(const hs_map_anchor_params& a) { return a.spacing >= 1; }
HS_HD inline uint64_t map_anchor_key(int32_t qa, int32_t t) { return ((uint64_t)(uint32_t)qa << 32) | (uint32_t)(0x7fffffff - t); }      // (qa, t >= 0)
HS_HD inline int32_t map_anchor_qa(uint64_t key) { return (int32_t)(key >> 32); }
HS_HD inline int32_t map_anchor_t(uint64_t key) { return 0x7fffffff - (int32_t)(uint32_t)key; }
HS_HD inline int32_t map_anchor_diag(uint64_t key) { return map_anchor_t(key) - map_anchor_qa(key); }
HS_HD inline int64_t map_anchor_bound(int64_t Lr, int32_t spacing) { return Lr / spacing + 1; }
// where read r's cut points are staged, from its offset in the concatenated reads alone: floor is superadditive, so the reads' rooms of
// map_anchor_bound do not overlap, and all of them end at or before map_anchor_stage_at(total bases, n_reads)
HS_HD inline int64_t map_anchor_stage_at(int64_t read_off, int64_t r, int32_t spacing) { return read_off / spacing + r; }
// are the ordered hits i - 1, i strictly increasing in t (then in qa as well: equal qa come with t descending)?
HS_HD inline bool map_anchor_rises(const uint64_t* keys, int i) { return map_anchor_t(keys[i - 1]) < map_anchor_t(keys[i]); }
// keys[0, n) ascending, n < HS_MAP_ANCHOR_NONE; tail and pred have room for n. Returns the chain's length, its members' indices ascending in tail[]
HS_HD inline int map_anchor_chain(const uint64_t* keys, int n, uint16_t* tail, uint16_t* pred) {
    int len = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t t = map_anchor_t(keys[i]);
        int lo = 0, hi = len;      // the first tail whose t is >= t
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (map_anchor_t(keys[tail[mid]]) < t) lo = mid + 1; else hi = mid; }
        pred[i] = lo ? tail[lo - 1] : (uint16_t)HS_MAP_ANCHOR_NONE;
        tail[lo] = (uint16_t)i;
        if (lo == len) ++len;
    }
    for (int j = len - 1; j > 0; --j) tail[j - 1] = pred[tail[j]];
    return len;
}
HS_HD inline bool map_anchor_supported(const uint64_t* keys, const uint16_t* chain, int len, int j) {
    const int32_t d = map_anchor_diag(keys[chain[j]]);
    return (j > 0 && map_anchor_diag(keys[chain[j - 1]]) == d) || (j + 1 < len && map_anchor_diag(keys[chain[j + 1]]) == d);
}
// the cut points over the supported members, sup[0, n) = their indices into keys in chain order: the first, then each time the first member whose qa
// is `spacing` or more above the last cut point's -- found by search, since qa rises strictly along a chain; the walk of the rule gives the same.
// At most cap are written (map_anchor_bound holds them all); returns their number
HS_HD inline int map_anchor_cuts(const uint64_t* keys, const uint16_t* sup, int n, int32_t spacing, int32_t* out_q, int32_t* out_t, int64_t cap) {
    int64_t m = 0;
    int j = 0;
    while (j < n) {
        const uint64_t key = keys[sup[j]];
        if (m < cap) { out_q[m] = map_anchor_qa(key); out_t[m] = map_anchor_t(key); }
        ++m;
        const int64_t want = (int64_t)map_anchor_qa(key) + spacing;
        int lo = j + 1, hi = n;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (map_anchor_qa(keys[sup[mid]]) < want) lo = mid + 1; else hi = mid; }
        j = lo;
    }
    return (int)(m < cap ? m : cap);
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
// the split form: segments in (read, span start) order, as hs_map_segments has them
struct MapSegmentsHost {
    std::vector<int64_t> seg_off;      // [n_reads + 1]
    std::vector<int32_t> read, contig, qstart, qend, tstart, tend, votes, second, round;
    std::vector<uint8_t> strand;
    std::vector<int32_t> n_minimizers, n_skipped, read_votes, read_second;      // per read
    std::vector<int64_t> n_hits;
};
int map_reads_split_host(const MapIndexHost& ix, const hs_map_split_params& sp, const uint8_t* read_seq, const int64_t* read_off, int32_t n_reads, int n_threads, MapSegmentsHost& out,
                         std::string& err);
// the anchored form: map_reads_host's result and the anchors of every read, as hs_map_anchors has them
struct MapAnchorsHost {
    std::vector<int64_t> anc_off;      // [n_reads + 1]
    std::vector<int32_t> anc_q, anc_t, n_best, n_chain, n_supported;
};
// the rule on the best's hits alone: keys = map_anchor_key of each (at most HS_MAP_ANCHOR_CAPACITY; sorted here), Lr the read's length. The cut
// points, the chain's length, its supported members and, where asked for, the chain's members as indices into the sorted keys
void map_anchors_of_keys(const hs_map_anchor_params& ap, int64_t Lr, std::vector<uint64_t>& keys, std::vector<int32_t>& q, std::vector<int32_t>& t, int32_t* n_chain,
                         int32_t* n_supported, std::vector<int32_t>* members);
int map_anchors_host(const MapIndexHost& ix, const hs_map_anchor_params& ap, const uint8_t* read_seq, const int64_t* read_off, int32_t n_reads, int n_threads, MapResultHost& out,
                     MapAnchorsHost& anchors, std::string& err);
// PAF lines of the mapped reads: names[] may be nullptr (then r<i> / c<i>)
std::string map_text(const hs_map_result* r, const char* const* read_names, const int64_t* read_len, const char* const* contig_names, const int64_t* contig_len);
// one PAF line per segment, in segment order: map_text's columns, then sg:i:<round> ns:i:<segments of the read>
std::string map_segments_text(const hs_map_segments* r, const char* const* read_names, const int64_t* read_len, const char* const* contig_names, const int64_t* contig_len);

}  // namespace hs
#endif
