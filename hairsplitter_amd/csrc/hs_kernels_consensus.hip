// hs_kernels_consensus.hip -- the consensus of a polishing bundle (hs_consensus_host.h states the rule): gfx950, wave64, plain
// vector stores and no-return atomics only. A round holds whole bundles; its columns are numbered through (g = the bundle's col_off + t, which
// is also the column's index in the round's backbone text).
//   k_cons_rows        pieces -> read-major rows: a wavefront per piece, lanes = CIGAR ops in 64-op chunks, prefix sums for the cursors; one byte
//                      per covered column (CONS_ROW_*), and the piece's voting insertions as records at the offsets the host's plan gave them
//   k_cons_columns     a workgroup per tile of 256 columns of one bundle, a lane per column: the bundle's rows that overlap the tile are read a
//                      byte a lane (256 consecutive bytes a row), the seven counters stay in registers; the column rule and the slot rule
//   k_cons_ins_vote    a lane per record: a record on a winning slot adds to the slot's table (lengths, then 4 counts per offset)
//   k_cons_ins_decide  a lane per column: the winning slot's length and bases; every column's output length
//   k_cons_emit        a lane per column: the text, behind the scan of the lengths
//   k_cons_bundles     a wavefront per bundle: its offsets, trim_* and counters
// For a caller whose pieces exist on the device only (hs_polish_haplotypes), in front of k_cons_rows:
//   k_cons_plan        a wavefront per piece: hs::cons_piece_plan on the device -- skipped?, covered columns, voting insertions, a CIGAR beyond 2^31 - 1;
//                      its bundle's row bytes, records and skipped pieces by no-return atomics
//   k_cons_layout      a lane per piece: the records k_cons_rows reads, rows and records at the offsets two scans of the plan gave
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_consensus_host.h"

namespace hsdev {

struct ConsPiece { int64_t base_off, cig_off, row_off, rec_off, col_off /* of its bundle */; int32_t n_ops, s0 /* first column */, n_cols /* 0: skipped */, n_rec; };
struct ConsBundle { int64_t col_off; int32_t piece0, piece1, L, ovl, ovr, pad; };
struct ConsTile { int32_t bundle, t0; };
struct ConsRecord { int64_t slot /* global column; -1: not written */, src; int32_t len, pad; };

__global__ __launch_bounds__(256) void k_cons_rows(const ConsPiece* __restrict__ pieces, int n_pieces, const uint32_t* __restrict__ cigar, const uint8_t* __restrict__ bases,
                                                   int32_t max_ins, uint8_t* __restrict__ rows, ConsRecord* __restrict__ recs) {
    const int lane = lane_id();
    const int p = (int)blockIdx.x * 4 + wave_id();
    if (p >= n_pieces) return;
    const ConsPiece pc = pieces[p];
    if (pc.n_cols <= 0) return;
    const uint32_t* __restrict__ cg = cigar + pc.cig_off;
    const uint8_t* __restrict__ txt = bases + pc.base_off;
    uint8_t* __restrict__ row = rows + pc.row_off;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int T = 0, Q = 0, I = 0, I_at_last = 0, n_rec = 0;      // column events, read bases and inserted bases so far; the inserted bases in front of the last column op
    bool any = false;                                      // a column event so far
    for (int k = 0; (k << 6) < pc.n_ops && T < pc.n_cols; ++k) {
        const int opi = (k << 6) + lane;
        const bool in_range = opi < pc.n_ops;
        const uint32_t op = in_range ? cg[opi] : 0u;
        const int code = (int)(op & 15u);
        const int a_col = (int)hs::cons_col_advance(op), a_rd = (int)hs::cons_read_advance(op), a_ins = code == 1 ? (int)(op >> 4) : 0;
        const int col_inc = wave_scan_incl(a_col), rd_inc = wave_scan_incl(a_rd), ins_inc = wave_scan_incl(a_ins);
        const int col_ex = T + col_inc - a_col, rd_ex = Q + rd_inc - a_rd, ins_ex = I + ins_inc - a_ins;
        // the insertion in front of a column op: the inserted bases since the column op before it
        const bool is_col = a_col > 0;
        const unsigned long long colmask = __ballot(is_col), below = colmask & lt_mask;
        const int src_lane = below ? 63 - __builtin_clzll(below) : lane;
        const int prev_ins = __shfl(ins_ex, src_lane, 64);
        const int ins_before = ins_ex - (below ? prev_ins : I_at_last);
        const bool has_ins = is_col && (below != 0 || any) && ins_before > 0 && col_ex < pc.n_cols;
        const unsigned long long recmask = __ballot(has_ins);
        const int ri = n_rec + __popcll(recmask & lt_mask);
        if (has_ins && ri < pc.n_rec) {
            ConsRecord r;
            r.slot = pc.col_off + pc.s0 + col_ex; r.src = pc.base_off + rd_ex - ins_before; r.len = hs::cons_ins_cap(ins_before, max_ins); r.pad = 0;
            recs[pc.rec_off + ri] = r;
        }
        n_rec += __popcll(recmask);
        // the chunk's column events, 64 at a time: the op of event e is the first lane whose inclusive count lies above it
        const int E = __builtin_amdgcn_readlane(col_inc, 63);
        const int end = T + E < pc.n_cols ? T + E : pc.n_cols;
        for (int e0 = T; e0 < end; e0 += 64) {
            const bool valid = e0 + lane < end;
            const int e = valid ? e0 + lane : end - 1;
            int lo = 0;
#pragma unroll
            for (int step = 32; step; step >>= 1) { const int v = __shfl(col_inc, lo + step - 1, 64); if (T + v <= e) lo += step; }
            const int j_code = __shfl(code, lo, 64), j_col = __shfl(col_ex, lo, 64), j_rd = __shfl(rd_ex, lo, 64), j_ins = __shfl((int)has_ins, lo, 64);
            if (valid) {
                const int off = e - j_col;
                const int vote = j_code == 0 ? hs::cons_code(txt[j_rd + off]) : hs::CONS_DEL;
                row[e] = (uint8_t)(vote | (off == 0 && j_ins ? hs::CONS_ROW_INS : 0) | (e > 0 ? hs::CONS_ROW_PREV : 0));
            }
        }
        if (colmask) { any = true; I_at_last = __shfl(ins_ex, 63 - __builtin_clzll(colmask), 64); }
        T += E; Q += __builtin_amdgcn_readlane(rd_inc, 63); I += __builtin_amdgcn_readlane(ins_inc, 63);
    }
}

// ---- the plan of a piece on the device (hs::cons_piece_plan is the rule): for a caller whose clipped CIGARs exist on the device only.
// A piece goes in as a ConsPiece whose row_off holds the index of its bundle, n_cols its base count and n_rec its piece_flags (the kernels
// above never see these records: k_cons_layout writes theirs). Sums of up to 2^31 ops of up to 2^28 run in 64 bits: a wave's 64 lengths are
// scanned as two 32-bit scans, of their low 16 bits and of the rest.
struct ConsPlan { int32_t skipped, long_cigar, n_cols, n_ins; };
struct ConsBundlePlan { long long row_bytes, n_rec; };

static __device__ __forceinline__ long long wave_scan_incl_i64(uint32_t len) {
    const int lo = wave_scan_incl((int)(len & 0xffffu)), hi = wave_scan_incl((int)(len >> 16));
    return ((long long)hi << 16) + (long long)lo;
}

// one wavefront per piece, lanes = CIGAR ops in 64-op chunks (the layout of k_cons_rows). A voting insertion: a column op of length > 0 with
// inserted bases behind the column op before it, a column event before it, and its first column inside the room L - s0. Whether inserted
// bases lie between two column ops is read off the ballots; `any` and `ins_open` carry it over a chunk's edge.
__global__ __launch_bounds__(256) void k_cons_plan(const ConsPiece* __restrict__ pieces, int n_pieces, const ConsBundle* __restrict__ bundles, const uint32_t* __restrict__ cigar,
                                                   ConsPlan* __restrict__ plan, int32_t* __restrict__ cols, int32_t* __restrict__ recs, ConsBundlePlan* __restrict__ bundle_plan,
                                                   int32_t* __restrict__ bundle_skipped, int32_t* __restrict__ first_long) {
    const int lane = lane_id();
    const int p = (int)blockIdx.x * 4 + wave_id();
    if (p >= n_pieces) return;
    const ConsPiece pc = pieces[p];
    const int b = (int)pc.row_off;
    const long long L = bundles[b].L, n_bases = pc.n_cols, room = L - pc.s0;
    const int32_t flags = pc.n_rec;
    const uint32_t* __restrict__ cg = cigar + pc.cig_off;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    long long T = 0, Q = 0;       // column events and read bases so far
    bool any = false;             // a column op of length > 0 so far
    bool ins_open = false;        // inserted bases behind the last column op (or, without one, behind the start)
    int n_ins = 0;
    for (int k = 0; (k << 6) < pc.n_ops; ++k) {
        const int opi = (k << 6) + lane;
        const uint32_t op = opi < pc.n_ops ? cg[opi] : 0u;
        const uint32_t a_col = (uint32_t)hs::cons_col_advance(op), a_rd = (uint32_t)hs::cons_read_advance(op);
        const long long col_inc = wave_scan_incl_i64(a_col), rd_inc = wave_scan_incl_i64(a_rd);
        const long long col_ex = T + col_inc - a_col;
        const bool is_col = a_col > 0;
        const unsigned long long colmask = __ballot(is_col), insmask = __ballot((op & 15u) == 1u && (op >> 4) > 0u), below = colmask & lt_mask;
        // the inserted bases between the column op before this lane and this lane
        const unsigned long long since = below ? ~((2ull << (63 - __builtin_clzll(below))) - 1ull) : ~0ull;
        const bool pending = (insmask & lt_mask & since) != 0ull || (!below && ins_open);
        const bool votes = is_col && pending && (below != 0ull || any) && col_ex < room;
        n_ins += __popcll(__ballot(votes));
        if (colmask) {
            const int last = 63 - __builtin_clzll(colmask);
            any = true;
            ins_open = last < 63 && (insmask >> (last + 1)) != 0ull;
        } else ins_open = ins_open || insmask != 0ull;
        T += __shfl(col_inc, 63, 64); Q += __shfl(rd_inc, 63, 64);
    }
    if (lane != 0) return;
    const bool long_cigar = T + Q > 0x7fffffffll;
    const bool skipped = long_cigar || n_bases == 0 || (flags & HS_POLISH_START_BEYOND_SEQ) || Q != n_bases || room <= 0;
    ConsPlan pl;
    pl.skipped = skipped ? 1 : 0; pl.long_cigar = long_cigar ? 1 : 0;
    pl.n_cols = skipped ? 0 : (int32_t)(T < room ? T : room); pl.n_ins = skipped ? 0 : n_ins;
    plan[p] = pl; cols[p] = pl.n_cols; recs[p] = pl.n_ins;
    if (long_cigar) __hip_atomic_fetch_min(first_long, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (skipped) __hip_atomic_fetch_add(&bundle_skipped[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else {
        __hip_atomic_fetch_add(&bundle_plan[b].row_bytes, (long long)pl.n_cols, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pl.n_ins) __hip_atomic_fetch_add(&bundle_plan[b].n_rec, (long long)pl.n_ins, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the pieces [p0, p0 + n) of a planned call as the records k_cons_rows and k_cons_columns read: rows and records at the scans' offsets, every
// offset counted from where the range begins (base0, cig0, col0; bundle0: the range's first bundle, whose column offset and rows come first)
__global__ __launch_bounds__(256) void k_cons_layout(const ConsPiece* __restrict__ src, long long p0, int n, const int32_t* __restrict__ cols, const int32_t* __restrict__ recs,
                                                     const int64_t* __restrict__ col_scan, const int64_t* __restrict__ rec_scan, long long base0, long long cig0, long long col0,
                                                     ConsPiece* __restrict__ dst) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const ConsPiece s = src[p0 + i];
    ConsPiece d;
    d.base_off = s.base_off - base0; d.cig_off = s.cig_off - cig0; d.col_off = s.col_off - col0;
    d.row_off = col_scan[p0 + i] - col_scan[p0]; d.rec_off = rec_scan[p0 + i] - rec_scan[p0];
    d.n_ops = s.n_ops; d.s0 = s.s0; d.n_cols = cols[p0 + i]; d.n_rec = recs[p0 + i];
    dst[i] = d;
}

__global__ __launch_bounds__(256) void k_cons_columns(const ConsTile* __restrict__ tiles, const ConsBundle* __restrict__ bundles, const ConsPiece* __restrict__ pieces,
                                                      const uint8_t* __restrict__ rows, const uint8_t* __restrict__ backbone, int32_t min_cov,
                                                      uint8_t* __restrict__ col, int32_t* __restrict__ slot_flag) {
    const ConsTile tl = tiles[blockIdx.x];
    const ConsBundle bu = bundles[tl.bundle];
    const int t = tl.t0 + (int)threadIdx.x;
    const bool active = t < bu.L;
    uint32_t v[5] = {0, 0, 0, 0, 0}, nins = 0, span = 0;
    for (int p = bu.piece0; p < bu.piece1; ++p) {
        const int s0 = pieces[p].s0, n = pieces[p].n_cols;
        if (n <= 0 || s0 >= tl.t0 + 256 || (int64_t)s0 + n <= tl.t0) continue;      // (uniform)
        const int rel = t - s0;
        if (!active || rel < 0 || rel >= n) continue;
        const uint32_t b = rows[pieces[p].row_off + rel];
        const uint32_t vote = b & hs::CONS_ROW_VOTE;
        v[0] += vote == 0; v[1] += vote == 1; v[2] += vote == 2; v[3] += vote == 3; v[4] += vote == 4;
        nins += (b & hs::CONS_ROW_INS) != 0; span += (b & hs::CONS_ROW_PREV) != 0;
    }
    if (!active) return;
    const int64_t g = bu.col_off + t;
    const bool wins = hs::cons_slot_wins(nins, span, min_cov);
    col[g] = (uint8_t)(hs::cons_column_byte(v, backbone[g], min_cov) | (wins ? hs::CONS_COL_SLOT : 0));
    slot_flag[g] = wins ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_cons_ins_vote(const ConsRecord* __restrict__ recs, long long n_recs, const uint8_t* __restrict__ col, const int64_t* __restrict__ slot_index,
                                                       long long n_slots, const uint8_t* __restrict__ bases, int32_t max_ins, uint32_t* __restrict__ tab) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_recs) return;
    const ConsRecord rec = recs[r];
    if (rec.slot < 0 || !(col[rec.slot] & hs::CONS_COL_SLOT)) return;
    const int64_t idx = slot_index[rec.slot];
    if (idx < 0 || idx >= n_slots || rec.len < 1 || rec.len > max_ins) return;
    uint32_t* __restrict__ t = tab + idx * hs::cons_table_words(max_ins);
    __hip_atomic_fetch_add(&t[rec.len], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int j = 0; j < rec.len; ++j)
        __hip_atomic_fetch_add(&t[max_ins + 1 + 4 * j + hs::cons_code(bases[rec.src + j])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_cons_ins_decide(const uint8_t* __restrict__ col, long long n_cols, const int64_t* __restrict__ slot_index, long long n_slots,
                                                         const uint32_t* __restrict__ tab, int32_t max_ins, int32_t* __restrict__ ins_len, uint8_t* __restrict__ ins_text,
                                                         int32_t* __restrict__ out_len) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_cols) return;
    const uint32_t c = col[g];
    int len = (c & hs::CONS_COL_CODE) == hs::CONS_DEL ? 0 : 1;
    if (c & hs::CONS_COL_SLOT) {
        const int64_t idx = slot_index[g];
        if (idx >= 0 && idx < n_slots) {
            const uint32_t* __restrict__ t = tab + idx * hs::cons_table_words(max_ins);
            const int l = hs::cons_ins_length(t, max_ins);
            for (int j = 0; j < l; ++j) ins_text[idx * max_ins + j] = hs::cons_letter(hs::cons_ins_base(t, max_ins, j));
            ins_len[idx] = l;
            len += l;
        }
    }
    out_len[g] = len;
}

__global__ __launch_bounds__(256) void k_cons_emit(const uint8_t* __restrict__ col, long long n_cols, const uint8_t* __restrict__ backbone, const int64_t* __restrict__ slot_index,
                                                   long long n_slots, const int32_t* __restrict__ ins_len, const uint8_t* __restrict__ ins_text, int32_t max_ins,
                                                   const int64_t* __restrict__ out_off, long long out_cap, uint8_t* __restrict__ out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_cols) return;
    const uint32_t c = col[g], w = c & hs::CONS_COL_CODE;
    int64_t o = out_off[g];
    if (c & hs::CONS_COL_SLOT) {
        const int64_t idx = slot_index[g];
        if (idx >= 0 && idx < n_slots) {
            const int l = ins_len[idx];
            for (int j = 0; j < l && j < max_ins; ++j, ++o) if (o >= 0 && o < out_cap) out[o] = ins_text[idx * max_ins + j];
        }
    }
    if (w != hs::CONS_DEL && o >= 0 && o < out_cap) out[o] = w == hs::CONS_KEEP ? backbone[g] : hs::cons_letter((int)w);
}

// per bundle: [0] its offset in the round's text is out_off[col_off]; v = trim_start, trim_end, n_sub, n_del, n_ins_bases, n_low
__global__ __launch_bounds__(256) void k_cons_bundles(const ConsBundle* __restrict__ bundles, int n_bundles, const uint8_t* __restrict__ col, const int64_t* __restrict__ slot_index,
                                                      long long n_slots, const int32_t* __restrict__ ins_len, const int64_t* __restrict__ out_off,
                                                      int64_t* __restrict__ cons_off, int32_t* __restrict__ v /* [6][n_bundles] */) {
    const int lane = lane_id();
    const int b = (int)blockIdx.x * 4 + wave_id();
    if (b >= n_bundles) return;
    const ConsBundle bu = bundles[b];
    int n_sub = 0, n_del = 0, n_ib = 0, n_low = 0;
    for (int t = lane; t < bu.L; t += 64) {
        const uint32_t c = col[bu.col_off + t], w = c & hs::CONS_COL_CODE;
        n_sub += (c & hs::CONS_COL_SUB) != 0; n_del += w == hs::CONS_DEL; n_low += w == hs::CONS_KEEP;
        if (c & hs::CONS_COL_SLOT) { const int64_t idx = slot_index[bu.col_off + t]; if (idx >= 0 && idx < n_slots) n_ib += ins_len[idx]; }
    }
    n_sub = wave_sum_i32(n_sub); n_del = wave_sum_i32(n_del); n_ib = wave_sum_i32(n_ib); n_low = wave_sum_i32(n_low);
    if (lane == 0) {
        const int64_t base = out_off[bu.col_off];
        const int c_start = bu.ovl < bu.L ? bu.ovl : bu.L, c_end = bu.L - (bu.ovr < bu.L ? bu.ovr : bu.L);
        cons_off[b] = base;
        if (b == n_bundles - 1) cons_off[n_bundles] = out_off[bu.col_off + bu.L];
        v[0 * (int64_t)n_bundles + b] = (int32_t)(out_off[bu.col_off + c_start] - base);
        v[1 * (int64_t)n_bundles + b] = (int32_t)(out_off[bu.col_off + c_end] - base);
        v[2 * (int64_t)n_bundles + b] = n_sub; v[3 * (int64_t)n_bundles + b] = n_del; v[4 * (int64_t)n_bundles + b] = n_ib; v[5 * (int64_t)n_bundles + b] = n_low;
    }
}

}  // namespace hsdev
