// hs_kernels_realign.hip -- the two device steps around A1 on the CIGAR-less route (hs_capi_realign.inc): the cut of the (read
// segment, contig window) pairs out of the job's resident sequences, and the conversion of the moves hs_edlib_hw_align leaves into
// the packed CIGAR words (len << 4 | op) hs_cv_batch_create takes -- what hs_realign.cpp does on the host threads (:105-115 the cut,
// :135-146 the runs) after bringing one byte per move across. gfx950, wave64; no LDS, plain vector loads and stores only.
//
// Moves to words: the unit of work is a CHUNK of M2C_CHUNK = 1024 consecutive moves of one pair (a wavefront: 64 lanes x 16 bytes),
// not a pair, so a 100-base and a 100-kb path fill wavefronts alike. A move begins a run when the move before it is of another
// class -- the only thing a chunk needs from outside is the byte before it. k_m2c_count leaves per chunk the number of words that
// begin in it (its runs, plus the clip words of the pair in its first and last chunk) and the place of its first run start; the
// exclusive scan of the counts (k_scan_*, hs_kernels_graph.hip) says where a chunk's words go; k_m2c_write finds every run start
// again with the same code (m2c_lane: both passes classify every byte through it, so a word cannot fall outside the counted range),
// and its end at the next start: in the lane, in the wavefront, or -- for the last start of a chunk -- in the first later chunk of
// the pair that has one (64 chunks per step), else at ops_len. A run over any number of chunks costs the chunk that begins it one
// such look; chunks without a start write nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hsdev {

enum { M2C_CHUNK = 1024, M2C_LANE = 16, M2C_NONE = 3 /* "no move before": differs from every class */ };

// 16 bytes from an arbitrary address as four dwords, only dwords that hold one of the `cnt` valid bytes are loaded
static __device__ __forceinline__ void load16_unaligned(const uint8_t* __restrict__ p, int cnt, uint32_t d[4]) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(p - sh);
    const int need = cnt > 0 ? (int)sh + cnt : 0;      // bytes from w[0] on
    uint32_t v[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) v[j] = 4 * j < need ? w[j] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], sh);
}

// the chunk's pair: the last i with chunk_first[i] <= c (pairs without room for a move own no chunk)
static __device__ __forceinline__ int m2c_pair_of(const int32_t* __restrict__ chunk_first, int n, int c) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (chunk_first[mid] <= c) lo = mid; else hi = mid - 1; }
    return lo;
}

// What one lane sees of its 16 moves. cls: their classes, two bits each (0 M, 1 I, 2 D); starts: bit 2 j set where move j begins a
// run; both are 0 beyond cnt.
struct M2cLane { uint32_t cls, starts; int cnt; };
static __device__ __forceinline__ uint32_t m2c_class(uint32_t b) { return b == 1u ? 1u : (b == 2u ? 2u : 0u); }
// moves: the pair's moves, len of them (> 0); k0: index of the chunk's first move; every lane of the wavefront calls it
static __device__ __forceinline__ M2cLane m2c_lane(const uint8_t* __restrict__ moves, int len, int k0, int lane) {
    M2cLane r;
    const int at = k0 + lane * M2C_LANE;
    r.cnt = len - at < 0 ? 0 : (len - at > M2C_LANE ? M2C_LANE : len - at);
    uint32_t d[4];
    load16_unaligned(moves + at, r.cnt, d);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < M2C_LANE; ++j) c |= m2c_class((d[j >> 2] >> (8 * (j & 3))) & 0xffu) << (2 * j);
    const uint32_t valid = r.cnt >= M2C_LANE ? 0xffffffffu : ((1u << (2 * r.cnt)) - 1u);
    c &= valid;
    // the class before the lane's first move: the last move of the lane below (full whenever this lane has a move), the byte before
    // the chunk for lane 0, none at the pair's first move
    const uint32_t last = r.cnt > 0 ? (c >> (2 * (r.cnt - 1))) & 3u : 0u;
    uint32_t prev = (uint32_t)__shfl_up((int)last, 1, 64);
    if (lane == 0) prev = k0 > 0 ? m2c_class(moves[k0 - 1]) : (uint32_t)M2C_NONE;
    const uint32_t x = c ^ ((c << 2) | prev);
    r.cls = c;
    r.starts = (x | (x >> 1)) & 0x55555555u & valid;
    return r;
}

struct M2cPair { int pair, k0 /* first move of the chunk */, len, clip_l, clip_r; bool first, last; };
// (wave-uniform) the chunk's pair, its moves clamped to the room the pair has, its clips, whether the chunk is its first / last with moves
static __device__ __forceinline__ M2cPair m2c_pair(int c, const int32_t* __restrict__ chunk_first, int n, const int64_t* __restrict__ ops_off,
                                                   const int32_t* __restrict__ ops_len, const int32_t* __restrict__ clip_left, const int32_t* __restrict__ clip_right) {
    M2cPair p;
    p.pair = m2c_pair_of(chunk_first, n, c);
    p.k0 = (c - chunk_first[p.pair]) * M2C_CHUNK;
    const int64_t room = ops_off[p.pair + 1] - ops_off[p.pair];
    const int l = ops_len[p.pair];
    p.len = l <= 0 ? 0 : ((int64_t)l > room ? (int)room : l);
    p.first = p.k0 == 0;
    p.last = p.len > 0 && p.k0 == ((p.len - 1) / M2C_CHUNK) * M2C_CHUNK;
    const int cl = clip_left ? clip_left[p.pair] : 0, cr = clip_right ? clip_right[p.pair] : 0;
    p.clip_l = cl > 0 ? cl : 0; p.clip_r = cr > 0 ? cr : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------
// k_m2c_count: per chunk the words that begin in it and the offset of its first run start (-1: none); per pair the reference span
// (M + D) and the read span (M + I + clips), added up chunk by chunk (spans zeroed by the caller; may be NULL)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_m2c_count(const uint8_t* __restrict__ ops, const int64_t* __restrict__ ops_off, const int32_t* __restrict__ ops_len,
                                                   const int32_t* __restrict__ clip_left, const int32_t* __restrict__ clip_right, int n,
                                                   const int32_t* __restrict__ chunk_first /* [n + 1] */, int n_chunks,
                                                   int32_t* __restrict__ chunk_cnt, int32_t* __restrict__ chunk_start, int32_t* __restrict__ spans) {
    const int lane = lane_id();
    const int c = (int)blockIdx.x * 4 + wave_id();
    if (c >= n_chunks) return;
    const M2cPair p = m2c_pair(c, chunk_first, n, ops_off, ops_len, clip_left, clip_right);
    if (p.k0 >= p.len) { if (lane == 0) { chunk_cnt[c] = 0; chunk_start[c] = -1; } return; }
    const M2cLane m = m2c_lane(ops + ops_off[p.pair], p.len, p.k0, lane);
    const int n_runs = wave_sum_i32(__popc(m.starts));
    const unsigned long long has = __ballot(m.starts != 0u);
    int first = -1;
    if (has) {
        const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(has));
        first = l * M2C_LANE + (__builtin_ctz(__builtin_amdgcn_readlane(m.starts, l)) >> 1);
    }
    const int n_i = wave_sum_i32(__popc(m.cls & 0x55555555u)), n_d = wave_sum_i32(__popc((m.cls >> 1) & 0x55555555u));
    const int n_all = (p.len - p.k0 < M2C_CHUNK ? p.len - p.k0 : M2C_CHUNK);
    if (lane == 0) {
        chunk_cnt[c] = n_runs + (p.first && p.clip_l ? 1 : 0) + (p.last && p.clip_r ? 1 : 0);
        chunk_start[c] = first;
        if (spans) {
            atomicAdd(&spans[2 * p.pair], n_all - n_i);                                                          // M + D
            atomicAdd(&spans[2 * p.pair + 1], n_all - n_d + (p.first ? p.clip_l : 0) + (p.last ? p.clip_r : 0));   // M + I + clips
        }
    }
}

// where the words of every pair begin: those of its first chunk (the next pair's when it has none)
__global__ __launch_bounds__(256) void k_m2c_pair_off(const int32_t* __restrict__ chunk_first, int n, const int64_t* __restrict__ chunk_woff, int64_t* __restrict__ word_off) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i <= n) word_off[i] = chunk_woff[chunk_first[i]];
}

// ------------------------------------------------------------------------------------------------
// k_m2c_write: the words of every chunk at chunk_woff[c] .. chunk_woff[c + 1]: nothing is stored outside that range
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_m2c_write(const uint8_t* __restrict__ ops, const int64_t* __restrict__ ops_off, const int32_t* __restrict__ ops_len,
                                                   const int32_t* __restrict__ clip_left, const int32_t* __restrict__ clip_right, int n,
                                                   const int32_t* __restrict__ chunk_first, int n_chunks, const int32_t* __restrict__ chunk_start,
                                                   const int64_t* __restrict__ chunk_woff, uint32_t* __restrict__ words) {
    const int lane = lane_id();
    const int c = (int)blockIdx.x * 4 + wave_id();
    if (c >= n_chunks) return;
    int64_t w0 = chunk_woff[c], w1 = chunk_woff[c + 1];
    if (w0 >= w1) return;
    const M2cPair p = m2c_pair(c, chunk_first, n, ops_off, ops_len, clip_left, clip_right);
    if (p.k0 >= p.len) return;
    if (p.first && p.clip_l) { if (lane == 0) words[w0] = ((uint32_t)p.clip_l << 4) | 4u; ++w0; }
    if (p.last && p.clip_r) { --w1; if (lane == 0 && w1 >= w0) words[w1] = ((uint32_t)p.clip_r << 4) | 4u; }
    const M2cLane m = m2c_lane(ops + ops_off[p.pair], p.len, p.k0, lane);
    const unsigned long long has = __ballot(m.starts != 0u);
    if (!has) return;
    // where the run of the chunk's last start ends: the first start of a later chunk of the pair, else the end of the moves
    int after = p.len;
    {
        const int cb = chunk_first[p.pair], c_last = cb + (p.len - 1) / M2C_CHUNK;
        for (int q = c + 1; q <= c_last; q += 64) {
            const int s = q + lane <= c_last ? chunk_start[q + lane] : -1;
            const unsigned long long hit = __ballot(s >= 0);
            if (hit) {
                const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(hit));
                after = (q + l - cb) * M2C_CHUNK + __builtin_amdgcn_readlane(s, l);
                break;
            }
        }
    }
    // the lane's first start and the first start above the lane (all in moves of the pair)
    const int mine = p.k0 + lane * M2C_LANE + (m.starts ? __builtin_ctz(m.starts) >> 1 : 0);
    const unsigned long long above = lane == 63 ? 0ull : has & ~((2ull << lane) - 1ull);
    const int theirs = __shfl(mine, above ? __builtin_ctzll(above) : lane, 64);
    const int lane_end = above ? theirs : after;
    const int n_mine = __popc(m.starts);
    int64_t w = w0 + (wave_scan_incl(n_mine) - n_mine);
    uint32_t s = m.starts;
    while (s) {
        const int j = __builtin_ctz(s) >> 1;
        s &= s - 1u;
        const int begin = p.k0 + lane * M2C_LANE + j;
        const int end = s ? p.k0 + lane * M2C_LANE + (__builtin_ctz(s) >> 1) : lane_end;
        if (w < w1) words[w] = ((uint32_t)(end - begin) << 4) | ((m.cls >> (2 * j)) & 3u);
        ++w;
    }
}

// ------------------------------------------------------------------------------------------------
// k_realign_cut: the query or the target buffer of hs_edlib_hw_align from the resident sequences. Piece i is out[off[i], off[i + 1]):
// the bases seq[src[i]], seq[src[i] + 1], ... or, where rev[i] is set, the complements 3 - code of seq[src[i]], seq[src[i] - 1], ...
// (hs_realign.cpp:111-114). The pieces lie back to back at arbitrary byte offsets and may be a single base long. As in k_polish_gather
// a workgroup owns a 4096-byte aligned window of the output and a lane an aligned 16-byte block, which it always stores whole (one
// dwordx4; bytes beyond the last piece are 0): a block inside one piece takes five aligned source dwords funnel-shifted into place
// (seq has HS_SEQ_PAD readable bytes on both sides), a block over a piece boundary is assembled byte by byte.
// out_bytes: the buffer's length rounded up to 16.
// ------------------------------------------------------------------------------------------------
static __device__ __forceinline__ uint32_t complement4(uint32_t x) {      // (uint8_t)(3 - b) in every byte, no borrow between them
    return (0x83838383u - (x & 0x7f7f7f7fu)) ^ (~x & 0x80808080u);
}
// the last i in [lo, hi] with off[i] <= a (off[lo] <= a)
static __device__ __forceinline__ int cut_piece_of(const int64_t* __restrict__ off, int lo, int hi, int64_t a) {
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= a) lo = mid; else hi = mid - 1; }
    return lo;
}
__global__ __launch_bounds__(256) void k_realign_cut(const int64_t* __restrict__ off /* [m + 1] */, const int64_t* __restrict__ src, const uint8_t* __restrict__ rev /* may be NULL */,
                                                     int m, const uint8_t* __restrict__ seq, uint8_t* __restrict__ out, int64_t out_bytes) {
    const int64_t win = (int64_t)blockIdx.x << 12;
    const int64_t a = win + ((int64_t)threadIdx.x << 4);
    if (a >= out_bytes) return;
    const int64_t total = off[m];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (a < total) {
        // the pieces of the window's first and last byte (the same for the whole workgroup), then the lane's own among them
        const int p_lo = cut_piece_of(off, 0, m - 1, win);
        const int64_t win_last = win + 4095 < total - 1 ? win + 4095 : total - 1;
        const int p_hi = cut_piece_of(off, p_lo, m - 1, win_last);
        int i = cut_piece_of(off, p_lo, p_hi, a);
        const bool r = rev && rev[i];
        if (a + 16 <= off[i + 1]) {
            const int64_t k = a - off[i];
            const int64_t p = r ? src[i] - k - 15 : src[i] + k;      // the 16 source bytes in ascending address order
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(seq + p) & 3u);
            const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(seq + p - sh);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
            const uint32_t d2 = __builtin_amdgcn_alignbyte(w3, w2, sh), d3 = __builtin_amdgcn_alignbyte(w4, w3, sh);
            if (r) {
                v.x = complement4(__builtin_amdgcn_perm(0u, d3, 0x00010203u)); v.y = complement4(__builtin_amdgcn_perm(0u, d2, 0x00010203u));
                v.z = complement4(__builtin_amdgcn_perm(0u, d1, 0x00010203u)); v.w = complement4(__builtin_amdgcn_perm(0u, d0, 0x00010203u));
            } else { v.x = d0; v.y = d1; v.z = d2; v.w = d3; }
        } else {
            uint32_t q[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; j < 16 && a + j < total; ++j) {
                while (a + j >= off[i + 1]) ++i;      // (a + j < total = off[m]: i stays below m)
                const int64_t k = a + j - off[i];
                const uint32_t b = rev && rev[i] ? (uint32_t)(uint8_t)(3 - seq[src[i] - k]) : (uint32_t)seq[src[i] + k];
                q[j >> 2] |= b << (8 * (j & 3));
            }
            v = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
    *reinterpret_cast<uint4*>(out + a) = v;
}

// POS of every pair: window start + start location (what hs_realign.cpp:134 prints, 0-based)
__global__ __launch_bounds__(256) void k_realign_pos(const int32_t* __restrict__ win0, const int32_t* __restrict__ start, int n, int32_t* __restrict__ pos) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < n) pos[i] = win0[i] + start[i];
}

// ------------------------------------------------------------------------------------------------
// The anchored route (hs_realign_intervals_anchored): an interval cut at its anchors is aligned as pieces -- a head (SHW on the two
// reversed strings), middles (NW), a tail (SHW), or one HW pair without anchors; a head or tail whose target is empty is a run of
// insertions and never reaches the aligner. The pieces of all intervals lie in one table in (interval, head .. tail) order; the three
// aligner calls leave their results in sections of the same arrays, so a piece names its moves by one offset and its numbers by one index.
//   k_anchor_join_plan   a lane per interval: where each piece's moves go inside the interval's string, their total, the summed distance
//                        and POS = the first anchor's t minus the target bases the head consumed (HW: window start + start location). An
//                        interval with a piece the aligner has no path for gets length -1 (no record, as on the plain route)
//   k_anchor_join        k_realign_cut's arrangement: a workgroup owns a 4096-byte aligned window of the joined strings, a lane an aligned
//                        16-byte block that it stores whole. A block inside one piece is one unaligned 16-byte load (a head's read
//                        backwards and its bytes turned), a block over a boundary is assembled byte by byte; bytes behind an interval's
//                        moves are 0. The joined strings lie at the host's offsets (an interval's room = query + window bases), as
//                        k_m2c_count / k_m2c_write take them.
// ------------------------------------------------------------------------------------------------
enum { ANCHOR_HW = 0, ANCHOR_HEAD = 1, ANCHOR_MID = 2, ANCHOR_TAIL = 3, ANCHOR_INS = 4 };
struct AnchorJoinArgs {
    int m;                              // intervals of the round
    const int32_t* iv_piece;            // [m + 1] an interval's pieces in the table
    const int32_t* iv_base;             // [m] the first anchor's t (no anchors: the window's start)
    const int64_t* join_off;            // [m + 1] where an interval's joined moves lie
    const uint8_t* pc_kind; const int32_t* pc_idx /* its numbers; ANCHOR_INS: the run's length */; const int32_t* pc_room /* moves it has room for */; const int64_t* pc_ops /* its moves in `ops` */;
    const uint8_t* ops; const int32_t* dist; const int32_t* start; const int32_t* end; const int32_t* len;
    int32_t* pc_at;                     // [pieces] where a piece's moves begin inside its interval's string
    int32_t* out_len; int32_t* out_dist; int32_t* out_pos;      // [m]
    uint8_t* joined; int64_t joined_bytes;      // rounded up to 16
};

__global__ __launch_bounds__(256) void k_anchor_join_plan(AnchorJoinArgs J) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k >= J.m) return;
    const int p0 = J.iv_piece[k], p1 = J.iv_piece[k + 1];
    const int64_t room = J.join_off[k + 1] - J.join_off[k];
    int64_t at = 0, dist = 0;
    bool ok = p1 > p0;
    int pos = J.iv_base[k];
    for (int p = p0; p < p1; ++p) {
        const int kind = J.pc_kind[p], i = J.pc_idx[p];
        int n = i;      // (ANCHOR_INS)
        if (kind != ANCHOR_INS) {
            n = J.len[i];
            dist += J.dist[i];
            if (kind == ANCHOR_HW) pos += J.start[i];
            if (kind == ANCHOR_HEAD) pos -= J.end[i] + 1;
        } else dist += n;
        ok = ok && n > 0 && n <= J.pc_room[p];
        J.pc_at[p] = (int32_t)at;
        at += n > 0 ? n : 0;
    }
    ok = ok && at <= room;      // (a path never has more moves than query + target bases)
    J.out_len[k] = ok ? (int32_t)at : -1; J.out_dist[k] = ok ? (int32_t)dist : -1; J.out_pos[k] = ok ? pos : -1;
}

// the last i in [lo, hi] with v[i] <= a (v[lo] <= a)
static __device__ __forceinline__ int join_last_le(const int32_t* __restrict__ v, int lo, int hi, int a) {
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (v[mid] <= a) lo = mid; else hi = mid - 1; }
    return lo;
}
// move x of interval k's string (0 <= x < out_len[k]), p = a piece at or before it
static __device__ __forceinline__ uint32_t join_byte(const AnchorJoinArgs& J, int p, int p1, int len_k, int x) {
    while (p + 1 < p1 && J.pc_at[p + 1] <= x) ++p;
    const int kind = J.pc_kind[p], in = x - J.pc_at[p];
    if (kind == ANCHOR_INS) return 1u;
    const int n = (p + 1 < p1 ? J.pc_at[p + 1] : len_k) - J.pc_at[p];
    return J.ops[J.pc_ops[p] + (kind == ANCHOR_HEAD ? n - 1 - in : in)];
}
__global__ __launch_bounds__(256) void k_anchor_join(AnchorJoinArgs J) {
    const int64_t win = (int64_t)blockIdx.x << 12;
    const int64_t a = win + ((int64_t)threadIdx.x << 4);
    if (a >= J.joined_bytes) return;
    const int64_t total = J.join_off[J.m];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (a < total) {
        int k = cut_piece_of(J.join_off, 0, J.m - 1, a);
        const int len_k = J.out_len[k];
        const int64_t x64 = a - J.join_off[k];
        const int p0 = J.iv_piece[k], p1 = J.iv_piece[k + 1];
        int p = p0;
        bool whole = false;
        if (len_k > 0 && x64 + 16 <= len_k) {
            p = join_last_le(J.pc_at, p0, p1 - 1, (int)x64);
            whole = (p + 1 < p1 ? J.pc_at[p + 1] : len_k) >= (int)x64 + 16;
        }
        if (whole) {
            const int kind = J.pc_kind[p], in = (int)x64 - J.pc_at[p];
            if (kind == ANCHOR_INS) v = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
            else {
                const int n = (p + 1 < p1 ? J.pc_at[p + 1] : len_k) - J.pc_at[p];
                uint32_t d[4];
                load16_unaligned(J.ops + J.pc_ops[p] + (kind == ANCHOR_HEAD ? n - 16 - in : in), 16, d);
                if (kind == ANCHOR_HEAD) {
                    v.x = __builtin_amdgcn_perm(0u, d[3], 0x00010203u); v.y = __builtin_amdgcn_perm(0u, d[2], 0x00010203u);
                    v.z = __builtin_amdgcn_perm(0u, d[1], 0x00010203u); v.w = __builtin_amdgcn_perm(0u, d[0], 0x00010203u);
                } else v = make_uint4(d[0], d[1], d[2], d[3]);
            }
        } else {
            uint32_t q[4] = {0u, 0u, 0u, 0u};
            int kk = k, lk = len_k, pp = p0, pe = p1;
            for (int j = 0; j < 16 && a + j < total; ++j) {
                if (a + j >= J.join_off[kk + 1]) {
                    while (a + j >= J.join_off[kk + 1]) ++kk;      // (a + j < total = join_off[m]: kk stays below m)
                    lk = J.out_len[kk]; pp = J.iv_piece[kk]; pe = J.iv_piece[kk + 1];
                }
                const int64_t x = a + j - J.join_off[kk];
                if (x >= lk) continue;
                if (j == 0 || x == 0) pp = join_last_le(J.pc_at, J.iv_piece[kk], pe - 1, (int)x);
                q[j >> 2] |= (join_byte(J, pp, pe, lk, (int)x) & 0xffu) << (8 * (j & 3));
            }
            v = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
    *reinterpret_cast<uint4*>(J.joined + a) = v;
}

}  // namespace hsdev
