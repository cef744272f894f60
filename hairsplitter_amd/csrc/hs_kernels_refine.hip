// hs_kernels_refine.hip -- polishing passes (hs_refine_host.h states the rule): between two passes of hs_kernels_consensus.hip, on what the
// earlier one left on the device. gfx950, wave64, plain vector stores and no-return atomics only.
//   k_refine_windows   a lane per piece: its window [ws, we) in the round's consensus text from out_off (the scan behind k_cons_ins_decide) and ins_len
//                      through slot_index, by hs::refine_window; the lengths and sources of its pair (0 / 0: no pair goes to the aligner)
//   k_refine_gather    the coded queries or the coded targets as one contiguous buffer of pairs (A1 takes pair i as [off[i], off[i + 1]), so windows that
//                      overlap in the text are materialised). k_realign_cut's arrangement: a workgroup owns a 4096-byte aligned window of the output,
//                      a lane an aligned 16-byte block that it stores whole (one dwordx4; bytes behind the last pair are 0); a block inside one pair
//                      takes five aligned source dwords funnel-shifted into place, a block over a pair boundary is assembled byte by byte. The bytes
//                      become the codes 0..3 of hs::cons_code four at a time (three byte-wise compares per dword, no table).
//   k_refine_pieces    a lane per piece: the piece as k_cons_plan reads it for the next pass (first column ws, CIGAR = the words the k_m2c_* kernels
//                      wrote for its pair, or the one word of an empty window, or none), and the pass's sums by no-return atomics
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_refine_host.h"

namespace hsdev {

struct RefineWin { int64_t ws, we; };      // in the round's text; -1 / -1: no window
struct RefineSums { long long n_unaligned, sum_dist, move_bytes, pad; };

// src: the pieces as pass p - 1's plan read them (n_cols = the base count); laid: as its rows were laid out (n_cols = covered columns, 0: skipped)
__global__ __launch_bounds__(256) void k_refine_windows(const ConsPiece* __restrict__ src, const ConsPiece* __restrict__ laid, int n, const uint8_t* __restrict__ col,
                                                        const int64_t* __restrict__ slot_index, long long n_slots, const int32_t* __restrict__ ins_len,
                                                        const int64_t* __restrict__ out_off, RefineWin* __restrict__ win, int32_t* __restrict__ q_len, int32_t* __restrict__ t_len,
                                                        int64_t* __restrict__ q_src, int64_t* __restrict__ t_src) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const ConsPiece lp = laid[i];
    RefineWin w;
    w.ws = -1; w.we = -1;
    if (hs::refine_has_window(lp.n_cols <= 0, lp.n_cols)) {
        const int64_t g0 = lp.col_off + lp.s0;
        int64_t ins = 0;
        if (col[g0] & hs::CONS_COL_SLOT) { const int64_t idx = slot_index[g0]; if (idx >= 0 && idx < n_slots) ins = ins_len[idx]; }
        hs::refine_window(out_off[g0], ins, out_off[g0 + lp.n_cols], &w.ws, &w.we);
    }
    const int64_t tl = w.we - w.ws;
    const bool pair = w.ws >= 0 && tl > 0 && tl <= 0x7fffffff && src[i].n_cols > 0;
    win[i] = w;
    q_len[i] = pair ? src[i].n_cols : 0; t_len[i] = pair ? (int32_t)tl : 0;
    q_src[i] = lp.base_off; t_src[i] = w.ws < 0 ? 0 : w.ws;
}

// hs::cons_code of four bytes at once: 0x01 in every byte of x that equals c, then 3 - 3 [A] - 2 [C] - [G] (at most one of them per byte: no borrow)
static __device__ __forceinline__ uint32_t refine_eq4(uint32_t x, uint32_t c) {
    const uint32_t z = x ^ (c * 0x01010101u);
    const uint32_t nz = (((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z) & 0x80808080u;
    return (nz ^ 0x80808080u) >> 7;
}
static __device__ __forceinline__ uint32_t refine_code4(uint32_t x) {
    return 0x03030303u - 3u * refine_eq4(x, 'A') - 2u * refine_eq4(x, 'C') - refine_eq4(x, 'G');
}
// the last i in [lo, hi] with off[i] <= a (off[lo] <= a)
static __device__ __forceinline__ int refine_pair_of(const int64_t* __restrict__ off, int lo, int hi, int64_t a) {
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= a) lo = mid; else hi = mid - 1; }
    return lo;
}
// pair i is out[off[i], off[i + 1]) = the codes of seq[src[i] ...]; a pair may be empty. seq lies in a block that begins at a multiple of 4 at
// or before it and has 16 readable bytes behind its last byte. out_bytes: off[m] rounded up to 16.
__global__ __launch_bounds__(256) void k_refine_gather(const int64_t* __restrict__ off /* [m + 1] */, const int64_t* __restrict__ src, int m, const uint8_t* __restrict__ seq,
                                                       uint8_t* __restrict__ out, int64_t out_bytes) {
    const int64_t win = (int64_t)blockIdx.x << 12;
    const int64_t a = win + ((int64_t)threadIdx.x << 4);
    if (a >= out_bytes) return;
    const int64_t total = off[m];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (a < total) {
        const int p_lo = refine_pair_of(off, 0, m - 1, win);
        const int64_t win_last = win + 4095 < total - 1 ? win + 4095 : total - 1;
        const int p_hi = refine_pair_of(off, p_lo, m - 1, win_last);
        int i = refine_pair_of(off, p_lo, p_hi, a);      // (the last pair that begins at or before a: an empty one never is)
        if (a + 16 <= off[i + 1]) {
            const int64_t p = src[i] + (a - off[i]);
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(seq + p) & 3u);
            const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(seq + p - sh);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            v.x = refine_code4(__builtin_amdgcn_alignbyte(w1, w0, sh)); v.y = refine_code4(__builtin_amdgcn_alignbyte(w2, w1, sh));
            v.z = refine_code4(__builtin_amdgcn_alignbyte(w3, w2, sh)); v.w = refine_code4(__builtin_amdgcn_alignbyte(w4, w3, sh));
        } else {
            uint32_t q[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; j < 16 && a + j < total; ++j) {
                while (a + j >= off[i + 1]) ++i;      // (a + j < total = off[m]: i stays below m)
                q[j >> 2] |= (uint32_t)hs::cons_code(seq[src[i] + (a + j - off[i])]) << (8 * (j & 3));
            }
            v = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
    *reinterpret_cast<uint4*>(out + a) = v;
}

// pair_of[i]: the piece's pair among those that went to the aligner, or -1. word_off / dist / ops_len are the pairs'. words has n_words + n entries: the
// word of an empty window lies at n_words + i. bundle_shift: what src's bundle index (row_off) counts from. cons_off: where the bundles' texts begin.
__global__ __launch_bounds__(256) void k_refine_pieces(const ConsPiece* __restrict__ src, const ConsPiece* __restrict__ laid, int n, long long bundle_shift,
                                                       const RefineWin* __restrict__ win, const int32_t* __restrict__ pair_of, const int64_t* __restrict__ word_off,
                                                       long long n_words, const int32_t* __restrict__ dist, const int32_t* __restrict__ ops_len, const int64_t* __restrict__ cons_off,
                                                       uint32_t* __restrict__ words, ConsPiece* __restrict__ next, RefineSums* __restrict__ sums) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const ConsPiece s = src[i];
    const RefineWin w = win[i];
    const int64_t b = s.row_off - bundle_shift, text0 = cons_off[b];
    ConsPiece d;
    d.base_off = laid[i].base_off; d.row_off = b; d.rec_off = 0; d.col_off = text0;
    d.s0 = hs::refine_sam_pos(w.ws < 0 ? -1 : w.ws - text0) - 1; d.n_cols = s.n_cols; d.n_rec = s.n_rec;
    d.cig_off = 0; d.n_ops = 0;
    const int pi = pair_of[i];
    if (pi >= 0) {
        const int64_t w0 = word_off[pi], w1 = word_off[pi + 1];
        d.cig_off = w0; d.n_ops = (int32_t)(w1 - w0);
        const int32_t len = ops_len[pi];
        if (len <= 0) __hip_atomic_fetch_add(&sums->n_unaligned, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else {
            __hip_atomic_fetch_add(&sums->sum_dist, (long long)dist[pi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&sums->move_bytes, (long long)len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (w.ws >= 0 && w.we == w.ws && s.n_cols > 0) {
        words[n_words + i] = hs::refine_empty_word(s.n_cols);
        d.cig_off = n_words + i; d.n_ops = 1;
    }
    next[i] = d;
}

}  // namespace hsdev
