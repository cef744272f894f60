// hs_kernels_map.hip -- the read mapper on the device: minimizers of contigs and reads, the bucketed index of the contigs' minimizers, the hits
// of every read minimizer, and the vote over diagonal bins that names a read's contig window. The rule is stated once, in hs_map_host.h, and
// every kernel below ends in its functions (map_kmer, map_hit, map_beats, map_second_allowed, map_in_best, map_interval). gfx950, wave64;
// builtins and plain C++ only, plain vector stores only.
//
//   k_map_minimizers<false|true>   a workgroup owns 256 consecutive bases of the concatenated sequences plus a halo of w - 1 <= 31 on either side;
//                                  hashes and every window's minimum go through LDS; the count pass leaves one count per workgroup, the write
//                                  pass (behind exclusive_scan_launch) writes in (sequence, position) order
//   k_map_seq_ranges               the minimizer range of every sequence
//   k_map_bucket_count / _fill     the index: bucket = low bits of the hash; no-return atomics count, an atomic cursor fills (the order inside
//                                  a bucket differs from run to run and no result depends on it)
//   k_map_hits_count / _fill       one lane per read minimizer scans its bucket: occ(h), then (key, qa, t) into the read's range of the scratch
//   k_map_vote                     one workgroup per read: keys sorted in LDS (block_bitonic_sort of hs_device.h), runs of equal keys give n,
//                                  a run and its successor the score, a block maximum under the rule's total order best and second, a second
//                                  pass over the hits the four extremes. More than HS_MAP_LDS_KEYS hits: on a list for
//   k_map_vote_wide                the same in a slab of global scratch (always queued; an empty list ends it)
//   k_map_vote_split / _split_wide the opt-in split form, the same arrangement: up to max_segments rounds per read, each the vote over the hits that
//                                  overlap no seed span taken so far (spans and gap counters in LDS, the free hits' keys compacted by a ballot
//                                  prefix and an LDS cursor, only that many sorted); a round without a free hit costs one pass over the hits
//   k_map_seg_compact              the reads' staged segments side by side (behind exclusive_scan_launch over their counts)
//   k_map_anchors                  the opt-in anchors (hs_map_host.h, "anchors"), behind the vote and in k_map_vote_split's arrangement: a workgroup per
//                                  read compacts the best's (qa, t) into LDS (ballot prefix, LDS cursor), sorts them under the chain's order, tests
//                                  "t already strictly increasing" in parallel (else one lane runs the patience pass: tails and 16-bit predecessor
//                                  links in LDS), lays the supported members side by side in parallel (ballot prefix), and one lane finds each next
//                                  cut among them by search and writes the read's staging
//   k_map_anchor_compact           the staged cut points side by side (behind exclusive_scan_launch over their counts), a wavefront per read
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_map_host.h"
#include "hs_device.h"

#define HS_MAP_LDS_KEYS 4096        /* hits of a read whose keys one workgroup sorts in LDS (32 KB) */
#define HS_MAP_WIDE_BLOCKS 16       /* most workgroups (and slabs) of k_map_vote_wide */
#define HS_MAP_HALO 31              /* w - 1 at most */

namespace hsdev {

// the sequence that holds base g of the concatenation (0 <= g < off[n_seqs]; empty sequences hold none)
static __device__ __forceinline__ int map_seq_of(const int64_t* __restrict__ off, int n_seqs, long long g) {
    int lo = 0, hi = n_seqs - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (off[mid + 1] <= g) lo = mid + 1; else hi = mid; }
    return lo;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_map_minimizers(const uint8_t* __restrict__ seq, const int64_t* __restrict__ off, int n_seqs, long long total, int k, int w,
                                                        int32_t* __restrict__ blk_cnt, const int64_t* __restrict__ blk_off, long long n_out,
                                                        uint32_t* __restrict__ out_h, uint32_t* __restrict__ out_ps, int32_t* __restrict__ out_seq) {
    __shared__ uint64_t s_h[256 + 2 * HS_MAP_HALO];      // slot i = base g0 - HALO + i: its k-mer's hash, or all ones (no k-mer there, or a skipped one)
    __shared__ int32_t s_arg[256 + HS_MAP_HALO];         // the window that starts at slot i: the slot of its minimizer (-1: no window, or all skipped)
    __shared__ int32_t s_wave[4];
    const int tid = (int)threadIdx.x;
    const long long g0 = (long long)blockIdx.x * 256;
    for (int i = tid; i < 256 + 2 * HS_MAP_HALO; i += 256) {
        const long long g = g0 - HS_MAP_HALO + i;
        uint64_t v = ~0ull;
        if (g >= 0 && g < total) {
            const int s = map_seq_of(off, n_seqs, g);
            uint32_t h, sb;
            if (g + k <= off[s + 1] && hs::map_kmer(seq + g, k, &h, &sb)) v = h;
        }
        s_h[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < 256 + HS_MAP_HALO; i += 256) {
        const long long g = g0 - HS_MAP_HALO + i;
        int arg = -1;
        if (g >= 0 && g < total) {
            const int s = map_seq_of(off, n_seqs, g);
            const long long p = g - off[s], n = off[s + 1] - off[s] - k + 1;
            if (n >= 1 && p <= hs::map_last_window(n, w)) {
                const int len = (int)(n - p < w ? n - p : w);      // (a window never leaves its sequence)
                uint64_t best = ~0ull;
                for (int q = 0; q < len; ++q) { const uint64_t v = s_h[i + q]; if (v < best) { best = v; arg = i + q; } }      // (strict: the leftmost of equal hashes)
            }
        }
        s_arg[i] = arg;
    }
    __syncthreads();
    const int me = HS_MAP_HALO + tid;
    bool named = false;
    if (s_h[me] != ~0ull)
        for (int j = me - (w - 1); j <= me; ++j) named = named || s_arg[j] == me;
    const unsigned long long ballot = __ballot(named);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) s_wave[wave] = __popcll(ballot);
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) blk_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        return;
    }
    if (!named) return;
    long long o = blk_off[blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) o += s_wave[v];
    if (o < 0 || o >= n_out) return;      // never write beyond the count pass's total
    const long long g = g0 + tid;
    const int s = map_seq_of(off, n_seqs, g);
    uint32_t h = 0, sb = 0;
    (void)hs::map_kmer(seq + g, k, &h, &sb);
    out_h[o] = h; out_ps[o] = ((uint32_t)(g - off[s]) << 1) | sb; out_seq[o] = s;
}

// mz_off[s] = the first minimizer of a sequence >= s (mz_seq ascends), s = 0 .. n_seqs
__global__ __launch_bounds__(256) void k_map_seq_ranges(const int32_t* __restrict__ mz_seq, long long n, int n_seqs, int64_t* __restrict__ mz_off) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s > n_seqs) return;
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (mz_seq[mid] < s) lo = mid + 1; else hi = mid; }
    mz_off[s] = lo;
}

__global__ __launch_bounds__(256) void k_map_bucket_count(const uint32_t* __restrict__ h, long long n, uint32_t mask, int32_t* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[h[i] & mask], 1);
}
__global__ __launch_bounds__(256) void k_map_bucket_fill(const uint32_t* __restrict__ h, const uint32_t* __restrict__ ps, const int32_t* __restrict__ sq, long long n, uint32_t mask,
                                                         const int64_t* __restrict__ bucket_off, int32_t* __restrict__ cursor, uint32_t* __restrict__ e_h,
                                                         int32_t* __restrict__ e_c, uint32_t* __restrict__ e_ts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = h[i] & mask;
    const long long o = bucket_off[b] + atomicAdd(&cursor[b], 1);
    if (o < 0 || o >= bucket_off[b + 1] || o >= n) return;
    e_h[o] = h[i]; e_c[o] = sq[i]; e_ts[o] = ps[i];
}

struct MapIndexDev {
    const int64_t* bucket_off; const uint32_t* e_h; const int32_t* e_c; const uint32_t* e_ts; uint32_t mask; long long n_entries;
    const int64_t* contig_off; int n_contigs;
};

// occ(h) of every read minimizer: cnt = occ, or 0 beyond max_occ (then the read's n_skipped counts it)
__global__ __launch_bounds__(256) void k_map_hits_count(MapIndexDev X, const uint32_t* __restrict__ mz_h, const int32_t* __restrict__ mz_seq, long long n_mz, int n_reads, int max_occ,
                                                        int32_t* __restrict__ cnt, int32_t* __restrict__ n_skipped) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_mz) return;
    const uint32_t h = mz_h[i];
    long long e = X.bucket_off[h & X.mask], e1 = X.bucket_off[(h & X.mask) + 1];
    if (e < 0) e = 0;
    if (e1 > X.n_entries) e1 = X.n_entries;
    int occ = 0;
    for (; e < e1; ++e) occ += X.e_h[e] == h ? 1 : 0;
    const int r = mz_seq[i];
    if (occ > max_occ) { occ = 0; if (r >= 0 && r < n_reads) atomicAdd(&n_skipped[r], 1); }
    cnt[i] = occ;
}
// hits of every read, and the most any read has
__global__ __launch_bounds__(256) void k_map_read_hits(const int64_t* __restrict__ mz_off, const int64_t* __restrict__ hit_off, int n_reads, int64_t* __restrict__ n_hits,
                                                       int32_t* __restrict__ n_minimizers, unsigned long long* __restrict__ max_hits) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n_reads) return;
    const long long n = hit_off[mz_off[r + 1]] - hit_off[mz_off[r]];
    n_hits[r] = n; n_minimizers[r] = (int32_t)(mz_off[r + 1] - mz_off[r]);
    if (n > 0) atomicMax(max_hits, (unsigned long long)n);
}
__global__ __launch_bounds__(256) void k_map_hits_fill(MapIndexDev X, const uint32_t* __restrict__ mz_h, const uint32_t* __restrict__ mz_ps, const int32_t* __restrict__ mz_seq,
                                                       long long n_mz, const int64_t* __restrict__ read_off, int n_reads, hs_map_params P, const int32_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ hit_off, long long n_hits, uint64_t* __restrict__ hit_key, int32_t* __restrict__ hit_qa,
                                                       int32_t* __restrict__ hit_t) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_mz || cnt[i] == 0) return;
    const int r = mz_seq[i];
    if (r < 0 || r >= n_reads) return;
    const int32_t Lr = (int32_t)(read_off[r + 1] - read_off[r]);
    const uint32_t h = mz_h[i], ps = mz_ps[i];
    long long o = hit_off[i];
    long long o1 = hit_off[i + 1];
    if (o < 0) return;
    if (o1 > n_hits) o1 = n_hits;      // never write beyond the scratch
    long long e = X.bucket_off[h & X.mask], e1 = X.bucket_off[(h & X.mask) + 1];
    if (e < 0) e = 0;
    if (e1 > X.n_entries) e1 = X.n_entries;
    for (; e < e1 && o < o1; ++e) {
        if (X.e_h[e] != h) continue;
        const uint32_t ts = X.e_ts[e];
        int32_t qa;
        hit_key[o] = hs::map_hit(X.e_c[e], (int32_t)(ts >> 1), ts & 1u, (int32_t)(ps >> 1), ps & 1u, Lr, P, &qa);
        hit_qa[o] = qa; hit_t[o] = (int32_t)(ts >> 1);
        ++o;
    }
}

struct MapVoteArgs {
    const int64_t* mz_off; const int64_t* hit_off; const uint64_t* hit_key; const int32_t* hit_qa; const int32_t* hit_t; long long n_hits;
    const int64_t* read_off; const int64_t* contig_off; int n_contigs, n_reads;
    hs_map_params P;
    int32_t* contig; uint8_t* strand; int32_t* qstart; int32_t* qend; int32_t* tstart; int32_t* tend; int32_t* votes; int32_t* second;
    int32_t* wide_count; int32_t* wide_list;
    uint64_t* best_key;      // [n_reads] or null: where the vote leaves a read's best key for k_map_anchors
};

// the block's best (score, key) under the rule's order; every thread calls it and gets the result. sc == 0: no candidate
static __device__ void map_block_best(uint32_t& sc, uint64_t& key, uint32_t* s_sc, uint64_t* s_key) {
    const int tid = (int)threadIdx.x;
    s_sc[tid] = sc; s_key[tid] = key;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) {
            const uint32_t so = s_sc[tid + d]; const uint64_t ko = s_key[tid + d];
            if (so != 0 && (s_sc[tid] == 0 || hs::map_beats(so, ko, s_sc[tid], s_key[tid]))) { s_sc[tid] = so; s_key[tid] = ko; }
        }
        __syncthreads();
    }
    sc = s_sc[0]; key = s_key[0];
    __syncthreads();
}

// the vote over keys[0, n), which lie padded with all ones to n_pow2 behind a __syncthreads(): sorted here; best and its key, and `second` where it is
// asked for. Every thread calls it and gets the result. The one vote of k_map_vote and of every round of k_map_vote_split.
static __device__ void map_vote_keys(uint64_t* keys, int n, int n_pow2, bool want_second, hs::MapVote& v, uint32_t* s_sc, uint64_t* s_key) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    block_bitonic_sort(keys, n_pow2);
    // first index at or behind `from` whose key is above v
    auto upper = [&](uint64_t v, int from) { int lo = from, hi = n; while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] <= v) lo = mid + 1; else hi = mid; } return lo; };
    auto score = [&](int i) { const uint64_t key = keys[i]; const int e = upper(key, i + 1); return (uint32_t)(upper(key + 1, e) - i); };      // (the run and the run of the next bin lie side by side)
    {
        uint32_t sc = 0; uint64_t key = 0;
        for (int i = tid; i < n; i += nt) {
            if (i && keys[i] == keys[i - 1]) continue;
            const uint32_t s = score(i);
            if (sc == 0 || hs::map_beats(s, keys[i], sc, key)) { sc = s; key = keys[i]; }
        }
        map_block_best(sc, key, s_sc, s_key);
        v.best = sc; v.key = key;
    }
    if (v.best && want_second) {
        uint32_t sc = 0; uint64_t key = 0;
        for (int i = tid; i < n; i += nt) {
            if ((i && keys[i] == keys[i - 1]) || !hs::map_second_allowed(keys[i], v.key)) continue;
            const uint32_t s = score(i);
            if (s > sc) { sc = s; key = keys[i]; }
        }
        map_block_best(sc, key, s_sc, s_key);
        v.second = sc;
    }
}

// one read, by whichever kernel owns it (256 threads); false: more hits than `cap` keys -- not this route's
static __device__ bool map_vote_one(const MapVoteArgs& A, int r, uint64_t* keys, long long cap, uint32_t* s_sc, uint64_t* s_key, int32_t* s_ext) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    long long h0 = A.hit_off[A.mz_off[r]], h1 = A.hit_off[A.mz_off[r + 1]];
    if (h0 < 0 || h1 > A.n_hits || h1 < h0) h1 = h0 = 0;
    const long long n64 = h1 - h0;
    if (n64 > cap) return false;
    const int n = (int)n64;
    const int n_pow2 = pow2_at_least(n);
    for (int i = tid; i < n_pow2; i += nt) keys[i] = i < n ? A.hit_key[h0 + i] : ~0ull;
    if (tid < 4) s_ext[tid] = (tid & 1) ? INT32_MIN : INT32_MAX;      // qa_min, qa_max, t_min, t_max
    __syncthreads();
    hs::MapVote v;
    map_vote_keys(keys, n, n_pow2, true, v, s_sc, s_key);
    if (v.best) {
        int qa_min = INT32_MAX, qa_max = INT32_MIN, t_min = INT32_MAX, t_max = INT32_MIN;
        for (int i = tid; i < n; i += nt) {
            if (!hs::map_in_best(A.hit_key[h0 + i], v.key)) continue;
            const int qa = A.hit_qa[h0 + i], t = A.hit_t[h0 + i];
            qa_min = min(qa_min, qa); qa_max = max(qa_max, qa); t_min = min(t_min, t); t_max = max(t_max, t);
        }
        atomicMin(&s_ext[0], qa_min); atomicMax(&s_ext[1], qa_max); atomicMin(&s_ext[2], t_min); atomicMax(&s_ext[3], t_max);
        __syncthreads();
        v.qa_min = s_ext[0]; v.qa_max = s_ext[1]; v.t_min = s_ext[2]; v.t_max = s_ext[3];
    }
    if (tid == 0) {
        const int c = v.best ? hs::map_key_contig(v.key) : -1;
        const int32_t Lc = c >= 0 && c < A.n_contigs ? (int32_t)(A.contig_off[c + 1] - A.contig_off[c]) : 0;
        const int32_t Lr = (int32_t)(A.read_off[r + 1] - A.read_off[r]);
        hs::map_interval(A.P, v, Lr, Lc, &A.contig[r], &A.strand[r], &A.qstart[r], &A.qend[r], &A.tstart[r], &A.tend[r]);
        A.votes[r] = (int32_t)v.best; A.second[r] = (int32_t)v.second;
        if (A.best_key) A.best_key[r] = v.key;
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(256) void k_map_vote(MapVoteArgs A) {
    __shared__ uint64_t s_keys[HS_MAP_LDS_KEYS];
    __shared__ uint64_t s_key[256];
    __shared__ uint32_t s_sc[256];
    __shared__ int32_t s_ext[4];
    const int r = (int)blockIdx.x;
    if (r >= A.n_reads) return;
    if (!map_vote_one(A, r, s_keys, HS_MAP_LDS_KEYS, s_sc, s_key, s_ext) && threadIdx.x == 0) wide_list_push(A.wide_count, A.wide_list, A.n_reads, r);
}

__global__ __launch_bounds__(256) void k_map_vote_wide(MapVoteArgs A, uint64_t* __restrict__ slabs, long long slab_keys) {
    __shared__ uint64_t s_key[256];
    __shared__ uint32_t s_sc[256];
    __shared__ int32_t s_ext[4];
    const int n = min(*A.wide_count, A.n_reads);
    uint64_t* keys = slabs + (size_t)blockIdx.x * (size_t)slab_keys;
    for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) (void)map_vote_one(A, A.wide_list[i], keys, slab_keys, s_sc, s_key, s_ext);
}

// ---- split mappings (hs_map_host.h, "split mappings"): the vote repeated over the hits that overlap no seed span taken so far ----
#define HS_MAP_SEG_WORDS 10        /* a segment as it leaves: read contig strand qstart qend tstart tend votes second round */
struct MapSplitArgs {
    hs_map_split_params S;
    int32_t* seg_count;            // [n_reads]: segments of every read
    int32_t* staged;               // [n_reads * S.max_segments] segments of HS_MAP_SEG_WORDS words, a read's side by side in span order
    int32_t* read_votes; int32_t* read_second;      // round 0's vote (cleared before the launch: a read without a hit keeps the zeros)
};
struct MapSplitShared {
    int32_t a0[HS_MAP_MAX_SEGMENTS], a1[HS_MAP_MAX_SEGMENTS];      // the spans, in the order taken
    uint32_t cnt[HS_MAP_MAX_SEGMENTS + 1];                        // the best's free hits per gap
    int32_t n_free, stop;
    hs::MapSegment seg[HS_MAP_MAX_SEGMENTS];
};

// one read's rounds, by whichever kernel owns it (256 threads); false: more hits than `cap` keys -- not this route's. A round is one pass over the
// hits that compacts the free ones' keys (round 0: all of them, map_vote_one's load), and only where there are any: the sort of that many keys, the
// vote, a pass for the gap counters (from round 1 on: round 0 has one gap) and a pass for the extremes.
static __device__ bool map_split_one(const MapVoteArgs& A, const MapSplitArgs& B, int r, uint64_t* keys, long long cap, uint32_t* s_sc, uint64_t* s_key, int32_t* s_ext,
                                     MapSplitShared& sh) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, lane = tid & 63;
    long long h0 = A.hit_off[A.mz_off[r]], h1 = A.hit_off[A.mz_off[r + 1]];
    if (h0 < 0 || h1 > A.n_hits || h1 < h0) h1 = h0 = 0;
    const long long n64 = h1 - h0;
    if (n64 > cap) return false;
    const int n = (int)n64, k = A.P.k;
    const int32_t Lr = (int32_t)(A.read_off[r + 1] - A.read_off[r]);
    const int max_segments = min(max(B.S.max_segments, 1), HS_MAP_MAX_SEGMENTS);
    int n_spans = 0;      // (the same in every thread)
    for (int round = 0; round < max_segments; ++round) {
        if (tid == 0) sh.n_free = 0;
        if (tid <= HS_MAP_MAX_SEGMENTS) sh.cnt[tid] = 0;
        if (tid < 4) s_ext[tid] = (tid & 1) ? INT32_MIN : INT32_MAX;      // qa_min, qa_max, t_min, t_max
        __syncthreads();
        int n_free = n;
        if (n_spans == 0) {
            for (int i = tid; i < n; i += nt) keys[i] = A.hit_key[h0 + i];
        } else {
            for (int base = 0; base < n; base += nt) {      // (every lane takes every turn: the ballot)
                const int i = base + tid;
                bool is_free = false;
                uint64_t key = 0;
                if (i < n) {
                    key = A.hit_key[h0 + i];
                    is_free = hs::map_hit_free(sh.a0, sh.a1, n_spans, hs::map_hit_q(A.hit_qa[h0 + i], hs::map_key_rel(key), Lr, k), k);
                }
                const unsigned long long b = __ballot(is_free);
                int at = 0;
                if (lane == 0 && b) at = atomicAdd(&sh.n_free, __popcll(b));
                at = __shfl(at, 0, 64);
                if (is_free) keys[at + __popcll(b & ((1ull << lane) - 1ull))] = key;      // (at most n keys: within `cap`)
            }
            __syncthreads();
            n_free = sh.n_free;
        }
        if (n_free == 0) break;
        const int n_pow2 = pow2_at_least(n_free);
        for (int i = n_free + tid; i < n_pow2; i += nt) keys[i] = ~0ull;
        __syncthreads();
        hs::MapVote v;
        map_vote_keys(keys, n_free, n_pow2, round == 0, v, s_sc, s_key);
        if (round == 0 && tid == 0) { B.read_votes[r] = (int32_t)v.best; B.read_second[r] = (int32_t)v.second; }
        if (v.best < hs::map_round_threshold(A.P, B.S, round)) break;
        int g = 0;
        uint32_t n_seg = v.best;
        if (n_spans > 0) {
            for (int i = tid; i < n; i += nt) {
                const uint64_t key = A.hit_key[h0 + i];
                if (!hs::map_in_best(key, v.key)) continue;
                const int32_t q = hs::map_hit_q(A.hit_qa[h0 + i], hs::map_key_rel(key), Lr, k);
                if (hs::map_hit_free(sh.a0, sh.a1, n_spans, q, k)) atomicAdd(&sh.cnt[hs::map_hit_gap(sh.a1, n_spans, q)], 1u);
            }
            __syncthreads();
            g = hs::map_best_gap(sh.cnt, n_spans + 1);
            n_seg = sh.cnt[g];
        }
        int qa_min = INT32_MAX, qa_max = INT32_MIN, t_min = INT32_MAX, t_max = INT32_MIN;
        for (int i = tid; i < n; i += nt) {
            const uint64_t key = A.hit_key[h0 + i];
            if (!hs::map_in_best(key, v.key)) continue;
            const int qa = A.hit_qa[h0 + i];
            const int32_t q = hs::map_hit_q(qa, hs::map_key_rel(key), Lr, k);
            if (!hs::map_hit_free(sh.a0, sh.a1, n_spans, q, k) || hs::map_hit_gap(sh.a1, n_spans, q) != g) continue;
            const int t = A.hit_t[h0 + i];
            qa_min = min(qa_min, qa); qa_max = max(qa_max, qa); t_min = min(t_min, t); t_max = max(t_max, t);
        }
        atomicMin(&s_ext[0], qa_min); atomicMax(&s_ext[1], qa_max); atomicMin(&s_ext[2], t_min); atomicMax(&s_ext[3], t_max);
        __syncthreads();
        if (tid == 0) {
            hs::MapSegment s;
            s.key = v.key; s.n = n_seg; s.second = round == 0 ? v.second : 0u; s.round = round;
            s.qa_min = s_ext[0]; s.qa_max = s_ext[1]; s.t_min = s_ext[2]; s.t_max = s_ext[3];
            hs::map_seed_span(hs::map_key_rel(s.key), Lr, s.qa_min, (int64_t)s.qa_max + k, &s.a0, &s.a1);
            const bool stands = n_seg > 0 && hs::map_segment_stands(B.S, round, n_seg, s.qa_min, (int64_t)s.qa_max + k);
            if (stands) { sh.seg[n_spans] = s; sh.a0[n_spans] = s.a0; sh.a1[n_spans] = s.a1; }
            sh.stop = stands ? 0 : 1;
        }
        __syncthreads();
        if (sh.stop) break;
        ++n_spans;
    }
    if (tid == 0) {
        hs::map_segments_sort(sh.seg, n_spans);
        for (int i = 0; i < n_spans; ++i) {
            const int c = hs::map_key_contig(sh.seg[i].key);
            const int32_t Lc = c >= 0 && c < A.n_contigs ? (int32_t)(A.contig_off[c + 1] - A.contig_off[c]) : 0;
            int32_t contig, qs, qe, ts, te;
            uint8_t strand;
            hs::map_segment_interval(A.P, B.S, sh.seg, n_spans, i, Lr, Lc, &contig, &strand, &qs, &qe, &ts, &te);
            int32_t* o = B.staged + ((size_t)r * (size_t)max_segments + (size_t)i) * HS_MAP_SEG_WORDS;
            o[0] = r; o[1] = contig; o[2] = strand; o[3] = qs; o[4] = qe; o[5] = ts; o[6] = te; o[7] = (int32_t)sh.seg[i].n; o[8] = (int32_t)sh.seg[i].second; o[9] = sh.seg[i].round;
        }
        B.seg_count[r] = n_spans;
    }
    __syncthreads();      // (the wide route's next read finds the tables free)
    return true;
}

__global__ __launch_bounds__(256) void k_map_vote_split(MapVoteArgs A, MapSplitArgs B) {
    __shared__ uint64_t s_keys[HS_MAP_LDS_KEYS];
    __shared__ uint64_t s_key[256];
    __shared__ uint32_t s_sc[256];
    __shared__ int32_t s_ext[4];
    __shared__ MapSplitShared sh;
    const int r = (int)blockIdx.x;
    if (r >= A.n_reads) return;
    if (!map_split_one(A, B, r, s_keys, HS_MAP_LDS_KEYS, s_sc, s_key, s_ext, sh) && threadIdx.x == 0) wide_list_push(A.wide_count, A.wide_list, A.n_reads, r);
}

__global__ __launch_bounds__(256) void k_map_vote_split_wide(MapVoteArgs A, MapSplitArgs B, uint64_t* __restrict__ slabs, long long slab_keys) {
    __shared__ uint64_t s_key[256];
    __shared__ uint32_t s_sc[256];
    __shared__ int32_t s_ext[4];
    __shared__ MapSplitShared sh;
    const int n = min(*A.wide_count, A.n_reads);
    uint64_t* keys = slabs + (size_t)blockIdx.x * (size_t)slab_keys;
    for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) (void)map_split_one(A, B, A.wide_list[i], keys, slab_keys, s_sc, s_key, s_ext, sh);
}

// the staged segments of every read, side by side at the offsets the scan of seg_count gave
__global__ __launch_bounds__(256) void k_map_seg_compact(const int32_t* __restrict__ seg_count, const int64_t* __restrict__ seg_off, const int32_t* __restrict__ staged, int n_reads,
                                                         int max_segments, long long cap, int32_t* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n_reads * max_segments) return;
    const int r = (int)(idx / max_segments), j = (int)(idx % max_segments);
    if (j >= seg_count[r]) return;
    const long long o = seg_off[r] + j;
    if (o < 0 || o >= cap) return;      // never write beyond the staging's size
    for (int w = 0; w < HS_MAP_SEG_WORDS; ++w) out[o * HS_MAP_SEG_WORDS + w] = staged[idx * HS_MAP_SEG_WORDS + w];
}


// ---- anchors (hs_map_host.h, "anchors"): the cut points of every mapped read of the LDS route ----
static_assert(HS_MAP_ANCHOR_CAPACITY == HS_MAP_LDS_KEYS, "a read of the LDS route has anchors; a read of the wide route has none");
struct MapAnchorArgs {
    hs_map_anchor_params P;
    int32_t* stage_q; int32_t* stage_t; long long stage_cap;      // read r's cut points from map_anchor_stage_at on, map_anchor_bound of them at most
    int32_t* anc_count; int32_t* n_best; int32_t* n_chain; int32_t* n_supported;      // [n_reads]
};

__global__ __launch_bounds__(256) void k_map_anchors(MapVoteArgs A, MapAnchorArgs B) {
    __shared__ uint64_t s_keys[HS_MAP_LDS_KEYS];
    __shared__ uint16_t s_chain[HS_MAP_LDS_KEYS];      // the patience tails, then the chain's members (indices into s_keys)
    __shared__ uint16_t s_pred[HS_MAP_LDS_KEYS];       // predecessor links, then the supported members side by side
    __shared__ int32_t s_n, s_falls, s_len, s_w[4];
    const int r = (int)blockIdx.x;
    if (r >= A.n_reads) return;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, lane = tid & 63;
    long long h0 = A.hit_off[A.mz_off[r]], h1 = A.hit_off[A.mz_off[r + 1]];
    if (h0 < 0 || h1 > A.n_hits || h1 < h0) h1 = h0 = 0;
    const long long n64 = h1 - h0;
    if (A.contig[r] < 0 || n64 > HS_MAP_LDS_KEYS) {      // (the same in every thread) unmapped, or the wide route's: no anchors
        if (tid == 0) { B.anc_count[r] = 0; B.n_best[r] = 0; B.n_chain[r] = 0; B.n_supported[r] = 0; }
        return;
    }
    const int n = (int)n64;
    const uint64_t best = A.best_key[r];
    if (tid == 0) { s_n = 0; s_falls = 0; s_len = 0; }
    __syncthreads();
    for (int base = 0; base < n; base += nt) {      // (every lane takes every turn: the ballot)
        const int i = base + tid;
        bool in = false;
        uint64_t key = 0;
        if (i < n && hs::map_in_best(A.hit_key[h0 + i], best)) { in = true; key = hs::map_anchor_key(A.hit_qa[h0 + i], A.hit_t[h0 + i]); }
        const unsigned long long b = __ballot(in);
        int at = 0;
        if (lane == 0 && b) at = atomicAdd(&s_n, __popcll(b));
        at = __shfl(at, 0, 64);
        if (in) s_keys[at + __popcll(b & ((1ull << lane) - 1ull))] = key;      // (at most n keys)
    }
    __syncthreads();
    const int nb = s_n, n_pow2 = pow2_at_least(nb);
    for (int i = nb + tid; i < n_pow2; i += nt) s_keys[i] = ~0ull;
    __syncthreads();
    block_bitonic_sort(s_keys, n_pow2);
    bool falls = false;
    for (int i = 1 + tid; i < nb; i += nt) falls = falls || !hs::map_anchor_rises(s_keys, i);
    if (falls) atomicOr(&s_falls, 1);
    __syncthreads();
    if (!s_falls) {
        for (int i = tid; i < nb; i += nt) s_chain[i] = (uint16_t)i;
        if (tid == 0) s_len = nb;
    } else if (tid == 0) s_len = hs::map_anchor_chain(s_keys, nb, s_chain, s_pred);
    __syncthreads();
    const int len = s_len;
    int n_sup = 0;      // (the same in every thread) the supported members side by side in chain order, where the predecessor links were
    for (int base = 0; base < len; base += nt) {      // (every lane takes every turn: the ballot)
        const int j = base + tid;
        const bool s = j < len && hs::map_anchor_supported(s_keys, s_chain, len, j);
        const uint16_t me = j < len ? s_chain[j] : (uint16_t)0;
        const unsigned long long b = __ballot(s);
        if (lane == 0) s_w[tid >> 6] = __popcll(b);
        __syncthreads();
        int at = n_sup + __popcll(b & ((1ull << lane) - 1ull));
        for (int v = 0; v < (tid >> 6); ++v) at += s_w[v];
        if (s) s_pred[at] = me;      // (at <= j: within the chain's length)
        n_sup += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) {
        const long long Lr = A.read_off[r + 1] - A.read_off[r];
        const long long at = hs::map_anchor_stage_at(A.read_off[r], r, B.P.spacing);
        long long cap = hs::map_anchor_bound(Lr, B.P.spacing);
        if (at < 0 || at >= B.stage_cap) cap = 0; else if (at + cap > B.stage_cap) cap = B.stage_cap - at;      // never write beyond the staging
        B.anc_count[r] = cap > 0 ? hs::map_anchor_cuts(s_keys, s_pred, n_sup, B.P.spacing, B.stage_q + at, B.stage_t + at, cap) : 0;
        B.n_best[r] = nb; B.n_chain[r] = len; B.n_supported[r] = n_sup;
    }
}

// the staged cut points of every read, side by side at the offsets the scan of anc_count gave: a wavefront per read
__global__ __launch_bounds__(256) void k_map_anchor_compact(const int32_t* __restrict__ anc_count, const int64_t* __restrict__ anc_off, const int64_t* __restrict__ read_off, int n_reads,
                                                            int spacing, const int32_t* __restrict__ stage_q, const int32_t* __restrict__ stage_t, long long stage_cap, long long cap,
                                                            int32_t* __restrict__ out_q, int32_t* __restrict__ out_t) {
    const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (r >= n_reads) return;
    const long long at = hs::map_anchor_stage_at(read_off[r], r, spacing), o = anc_off[r];
    const int n = anc_count[r];
    for (int j = lane; j < n; j += 64) {
        if (at + j < 0 || at + j >= stage_cap || o + j < 0 || o + j >= cap) continue;      // never read or write beyond either block
        out_q[o + j] = stage_q[at + j]; out_t[o + j] = stage_t[at + j];
    }
}

}  // namespace hsdev
