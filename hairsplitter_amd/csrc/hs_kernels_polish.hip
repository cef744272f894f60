// hs_kernels_polish.hip -- the polisher's inputs of the reference's stage 5 (create_new_contigs.cpp:383-506, 517-519): for every
// merged interval of a contig and every read with a label above -1, the part of the read and of its CIGAR that lies over the
// interval plus its overhangs, and the backbone piece `toPolish`. gfx950, wave64; no LDS, plain vector stores only.
//
// The reference expands the CIGAR to one char per base (convert_cigar, tools.cpp:27-57) and walks the chars (:403-437). Here the
// ops stay run-length encoded: one wavefront owns one (interval, record) task, lanes are ops, and the walk starts at the 64-op chunk
// that holds leftToPolish, found by bisection on a per-chunk table of the walk's two cursors.
//
// That table is NOT K0's chunk_start (hs_kernels.hip, k_cigar_scan): K0 counts '=' and 'X' as matches and 'N' not at all, as
// call_variants.cpp does, whereas the walk of :403-437 knows M I D S H only -- '=' 'X' 'N' 'P' chars advance neither cursor
// (they are still chars of the CIGAR, and still places where the piece can begin or end). k_polish_scan builds the table with the
// walk's own rules, once per call, for the records of the call.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hsdev {

// per (interval, record) task: what the host hands to k_polish_cut
struct PolishTask { int32_t rec, left, right, pad; };
// what k_polish_cut returns per task (POLISH_* slots of 12 int32)
enum { PC_READ_START = 0, PC_READ_END, PC_OP_FIRST, PC_OFF_FIRST, PC_OP_LAST, PC_OFF_LAST, PC_N_OPS, PC_SAM_POS, PC_FLAGS, PC_LEN, PC_CHUNKS /* 64-op chunks the walk loaded */, PC_SLOTS = 12 };
enum { POLISH_DROPPED = 1, POLISH_START_BEYOND_SEQ = 2 };

// how far one op moves the read cursor and the reference cursor in the walk of :403-437 before the piece has begun
// (S and H both move the read cursor, :406-414; '=' 'X' 'N' 'P' match no branch)
static __device__ __forceinline__ void polish_advances(uint32_t op, bool in_range, int& rd, int& rf) {
    const int len = in_range ? (int)(op >> 4) : 0, code = (int)(op & 15u);
    rd = (code == 0 || code == 1 || code == 4 || code == 5) ? len : 0;
    rf = (code == 0 || code == 2) ? len : 0;
}

// the two cursors at every 64-op chunk boundary of a record: tab[2 * chunk] = read cursor, tab[2 * chunk + 1] = reference cursor
__global__ __launch_bounds__(256) void k_polish_scan(const int32_t* __restrict__ recs, int n, const int32_t* __restrict__ rec_pos,
                                                     const int64_t* __restrict__ rec_cig_off, const uint32_t* __restrict__ cigar,
                                                     const int64_t* __restrict__ chunk_off /* [n + 1], by position in recs */, int32_t* __restrict__ tab) {
    const int lane = lane_id();
    const int i = (int)blockIdx.x * 4 + wave_id();
    if (i >= n) return;
    const int r = recs[i];
    const int64_t cig0 = rec_cig_off[r], cig1 = rec_cig_off[r + 1];
    int32_t* __restrict__ t = tab + 2 * chunk_off[i];
    int rd_cur = 0, rf_cur = rec_pos[r], k = 0;
    for (int64_t ob = cig0; ob < cig1; ob += 64, ++k) {
        const int64_t oi = ob + lane;
        int rd, rf;
        polish_advances(oi < cig1 ? cigar[oi] : 0u, oi < cig1, rd, rf);
        if (lane == 0) { t[2 * k] = rd_cur; t[2 * k + 1] = rf_cur; }
        rd_cur += wave_sum_i32(rd); rf_cur += wave_sum_i32(rf);
    }
}

// One chunk of the clipped CIGAR, shared by k_polish_cut (which counts the runs) and k_polish_cigar (which writes them): the chars
// [first op + its offset, last op + its offset) re-encoded as runs (convert_cigar2, tools.cpp:61-80) -- neighbouring ops of one
// code fuse and ops without chars vanish. `eff` is the number of chars of the lane's op that lie in the range; a lane is the head
// of a run when the last op with chars before it (prev_code across chunks) has another code.
static __device__ __forceinline__ unsigned long long polish_run_heads(int lane, int eff, int code, int prev_code) {
    const bool nz = eff > 0;
    const unsigned long long nzm = __ballot(nz), below = nzm & ((1ull << lane) - 1ull);
    const int src = below ? 63 - __builtin_clzll(below) : lane;
    const int pc = __shfl(code, src, 64);
    return __ballot(nz && (below ? pc != code : prev_code != code));
}
static __device__ __forceinline__ int polish_eff_len(int64_t op_index, bool in_range, int len, int64_t op_first, int off_first, int64_t op_last, int off_last) {
    if (!in_range || op_index < op_first || op_index > op_last) return 0;
    int lo = op_index == op_first ? off_first : 0;
    int hi = op_index == op_last ? off_last : len;
    return hi > lo ? hi - lo : 0;
}

// ------------------------------------------------------------------------------------------------
// k_polish_cut: create_new_contigs.cpp:392-447 on the run-length ops. With S = the first non-clip char at which the reference
// cursor is >= left, E = the first non-clip char at which it == right and C = the first S/H char after S, the piece begins at S and
// ends at the earlier of E and C, or at the end of the walk; E before S leaves posOnReadStart at -1 and the read is dropped.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_polish_cut(const PolishTask* __restrict__ tasks, int n_tasks, const int32_t* __restrict__ slot_of_rec,
                                                    const int32_t* __restrict__ rec_pos, const int32_t* __restrict__ rec_read,
                                                    const int64_t* __restrict__ read_off, const int64_t* __restrict__ rec_cig_off,
                                                    const uint32_t* __restrict__ cigar, const int64_t* __restrict__ chunk_off,
                                                    const int32_t* __restrict__ tab, int32_t* __restrict__ out) {
    const int lane = lane_id();
    const int t = (int)blockIdx.x * 4 + wave_id();
    if (t >= n_tasks) return;
    const PolishTask task = tasks[t];
    const int r = task.rec, left = task.left, right = task.right;
    const int64_t cig0 = rec_cig_off[r], cig1 = rec_cig_off[r + 1];
    const int n_ops = (int)(cig1 - cig0), n_chunks = (n_ops + 63) >> 6;
    const int32_t* __restrict__ cs = tab + 2 * chunk_off[slot_of_rec[r]];
    const int rd_id = rec_read[r];
    const int rlen = (int)(read_off[rd_id + 1] - read_off[rd_id]);

    // last chunk that begins with the reference cursor below both bounds: no char before it can be S or E
    const int tgt = left < right ? left : right;
    int klo = 0, khi = n_chunks - 1;
    while (klo < khi) { const int mid = (klo + khi + 1) >> 1; if (cs[2 * mid + 1] < tgt) klo = mid; else khi = mid - 1; }

    bool started = false, ended = false, dropped = false;
    int rs = -1, re = -1, op_first = 0, off_first = 0, op_last = n_ops, off_last = 0, n_runs = 0, prev_code = -1, rd_end = 0, n_walked = 0;
    for (int k = klo; k < n_chunks && !ended && !dropped; ++k) {
        const int opi = (k << 6) + lane;
        const bool in_range = opi < n_ops;
        const uint32_t op = in_range ? cigar[cig0 + opi] : 0u;
        const int len = in_range ? (int)(op >> 4) : 0, code = (int)(op & 15u);
        ++n_walked;
        int a_rd, a_rf;
        polish_advances(op, in_range, a_rd, a_rf);
        const int rd_inc = wave_scan_incl(a_rd), rf_inc = wave_scan_incl(a_rf);
        const int rd_ex = cs[2 * k] + rd_inc - a_rd, rf_ex = cs[2 * k + 1] + rf_inc - a_rf;
        rd_end = cs[2 * k] + __builtin_amdgcn_readlane(rd_inc, 63);
        const bool clip = code == 4 || code == 5;
        const bool nonclip = in_range && !clip && len > 0;
        // offset of the op's first char that can be S / is E (chars of an op that does not move the reference cursor all sit at rf_ex)
        const bool s_here = nonclip && (rf_ex >= left || (a_rf > 0 && rf_ex + len > left));
        const int s_off = rf_ex >= left ? 0 : left - rf_ex;
        const bool e_here = nonclip && (a_rf > 0 ? (rf_ex <= right && right < rf_ex + len) : rf_ex == right);
        const int e_off = a_rf > 0 ? right - rf_ex : 0;
        unsigned long long em = __ballot(e_here), cm = __ballot(in_range && clip && len > 0);
        int lo_lane = 0;   // first lane of the chunk that belongs to the piece
        if (!started) {
            const unsigned long long sm = __ballot(s_here);
            const int ls = sm ? __builtin_amdgcn_readfirstlane(__builtin_ctzll(sm)) : 64;
            if (em) {   // an end before the start: the walk breaks with posOnReadStart == -1 (:421-425, :444)
                const int le = __builtin_amdgcn_readfirstlane(__builtin_ctzll(em));
                if (le < ls || (le == ls && __builtin_amdgcn_readlane(e_off, le) < __builtin_amdgcn_readlane(s_off, ls))) { dropped = true; break; }
            }
            if (ls == 64) continue;
            started = true;
            op_first = (k << 6) + ls; off_first = __builtin_amdgcn_readlane(s_off, ls);
            rs = __builtin_amdgcn_readlane(rd_ex, ls) + (__builtin_amdgcn_readlane(a_rd, ls) > 0 ? off_first : 0);
            lo_lane = ls;
            const unsigned long long from = ~0ull << ls;
            em &= from; cm &= from << 1;
        }
        const int le = em ? __builtin_ctzll(em) : 64, lc = cm ? __builtin_ctzll(cm) : 64;
        int hi_lane = 63;
        if (le < 64 || lc < 64) {
            ended = true;
            const int l = __builtin_amdgcn_readfirstlane(le < lc ? le : lc);
            op_last = (k << 6) + l; off_last = le < lc ? __builtin_amdgcn_readlane(e_off, l) : 0;
            re = __builtin_amdgcn_readlane(rd_ex, l) + (__builtin_amdgcn_readlane(a_rd, l) > 0 ? off_last : 0);
            hi_lane = l;
        }
        // runs of the clipped CIGAR that begin in this chunk
        const int eff = (lane < lo_lane || lane > hi_lane) ? 0 : polish_eff_len(opi, in_range, len, op_first, off_first, ended ? op_last : 0x7fffffff, off_last);
        n_runs += __popcll(polish_run_heads(lane, eff, code, prev_code));
        const unsigned long long nzm = __ballot(eff > 0);
        if (nzm) prev_code = __builtin_amdgcn_readlane(code, __builtin_amdgcn_readfirstlane(63 - __builtin_clzll(nzm)));
    }
    if (started && !ended && !dropped) re = rd_end;              // :439-442
    if (!started || rs > re) dropped = true;                     // :444-447
    if (lane == 0) {
        int32_t* __restrict__ o = out + (int64_t)t * PC_SLOTS;
        int flags = 0, plen = 0;
        if (dropped) flags = POLISH_DROPPED;
        else if (rs > rlen) flags = POLISH_START_BEYOND_SEQ;     // std::string::substr would throw (:459): an empty piece and a flag
        else plen = re - rs < rlen - rs ? re - rs : rlen - rs;   // substr clamps the count to the end of the string
        o[PC_READ_START] = dropped ? -1 : rs; o[PC_READ_END] = dropped ? -1 : re;
        o[PC_OP_FIRST] = op_first; o[PC_OFF_FIRST] = off_first; o[PC_OP_LAST] = op_last; o[PC_OFF_LAST] = off_last;
        o[PC_N_OPS] = dropped ? 0 : n_runs;
        const int sam = rec_pos[r] + 1 - left;
        o[PC_SAM_POS] = sam > 1 ? sam : 1;                       // :394-395
        o[PC_FLAGS] = flags; o[PC_LEN] = plen; o[PC_CHUNKS] = n_walked; o[11] = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// k_polish_cigar: the clipped CIGAR of every piece (:460-462) as packed len << 4 | op words. One wavefront per piece, lanes are
// ops; a run that crosses a chunk boundary is carried (wave-uniform) and written when it closes.
// ------------------------------------------------------------------------------------------------
struct PolishCigTask { int32_t rec, op_first, off_first, op_last, off_last, n_out /* words k_polish_cut counted: nothing is written beyond them */; int64_t out_off; };
__global__ __launch_bounds__(256) void k_polish_cigar(const PolishCigTask* __restrict__ tasks, int n_tasks, const int64_t* __restrict__ rec_cig_off,
                                                      const uint32_t* __restrict__ cigar, uint32_t* __restrict__ out) {
    const int lane = lane_id();
    const int t = (int)blockIdx.x * 4 + wave_id();
    if (t >= n_tasks) return;
    const PolishCigTask task = tasks[t];
    const int64_t cig0 = rec_cig_off[task.rec], cig1 = rec_cig_off[task.rec + 1];
    const int n_ops = (int)(cig1 - cig0);
    uint32_t* __restrict__ o = out + task.out_off;
    const int k1 = (task.op_last < n_ops ? task.op_last : n_ops - 1) >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int carry_len = 0, carry_code = -1, n_out = 0;
    for (int k = task.op_first >> 6; k <= k1; ++k) {
        const int opi = (k << 6) + lane;
        const bool in_range = opi < n_ops;
        const uint32_t op = in_range ? cigar[cig0 + opi] : 0u;
        const int len = in_range ? (int)(op >> 4) : 0, code = (int)(op & 15u);
        const int eff = polish_eff_len(opi, in_range, len, task.op_first, task.off_first, task.op_last, task.off_last);
        const unsigned long long hm = polish_run_heads(lane, eff, code, carry_code);
        const int p_inc = wave_scan_incl(eff), p_ex = p_inc - eff;
        const int total = __builtin_amdgcn_readlane(p_inc, 63);
        if (!hm) { carry_len += total; continue; }
        const int lf = __builtin_amdgcn_readfirstlane(__builtin_ctzll(hm)), ll = __builtin_amdgcn_readfirstlane(63 - __builtin_clzll(hm));
        const int before = __builtin_amdgcn_readlane(p_ex, lf);          // chars that still belong to the carried run
        if (carry_len + before > 0) { if (lane == 0 && n_out < task.n_out) o[n_out] = ((uint32_t)(carry_len + before) << 4) | (uint32_t)carry_code; ++n_out; }
        // every head but the last one of the chunk closes at the next head
        const unsigned long long above = hm & ~lt_mask & ~(1ull << lane);
        const int nh = above ? __builtin_ctzll(above) : lane;
        const int next_ex = __shfl(p_ex, nh, 64);
        if (((hm >> lane) & 1ull) && above && n_out + __popcll(hm & lt_mask) < task.n_out) o[n_out + __popcll(hm & lt_mask)] = ((uint32_t)(next_ex - p_ex) << 4) | (uint32_t)code;
        n_out += __popcll(hm) - 1;
        carry_len = total - __builtin_amdgcn_readlane(p_ex, ll);
        carry_code = __builtin_amdgcn_readlane(code, ll);
    }
    if (carry_len > 0 && lane == 0 && n_out < task.n_out) o[n_out] = ((uint32_t)carry_len << 4) | (uint32_t)carry_code;
}

// ------------------------------------------------------------------------------------------------
// k_polish_gather: the bases of every piece (:453-459) and of toPolish (:517-519). The sequences of the batch are codes 0..3 (the
// reference's Sequence, sequence.cpp:13-52: anything but A C G is T), one per byte; the output is text. A task is one 4096-byte
// aligned window of the output buffer, cut to one piece: 256 lanes, 16 output bytes each, so that a long piece is many tasks and
// every store of a whole 16-byte block is one aligned dwordx4. The source is read as aligned dwords and funnel-shifted into place;
// the reverse strand (:454-456) reads backwards, reverses the bytes and complements through the letter table.
// ------------------------------------------------------------------------------------------------
struct PolishPiece { int64_t out_off, src; int32_t len, rev; };   // src: index of the source byte of the piece's first base (rev: the bases before it follow)
struct PolishSlice { int32_t piece, window; };                    // window: index of the 4096-byte window of the output buffer

// codes -> letters, four at a time: v_perm_b32 looks the bytes 0..3 up in `table`; any other value is a T of the read (`other`: "TTTT",
// or its complement on the reverse strand)
static __device__ __forceinline__ uint32_t polish_letters(uint32_t codes, uint32_t table, uint32_t other) {
    const uint32_t high = codes & 0xFCFCFCFCu;
    const uint32_t nzb = ((high | ((high & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u) >> 7;   // 1 in every byte that is not 0..3
    const uint32_t sel = (codes & 0x03030303u) | (nzb << 2);
    return __builtin_amdgcn_perm(other, table, sel);
}

__global__ __launch_bounds__(256) void k_polish_gather(const PolishPiece* __restrict__ pieces, const PolishSlice* __restrict__ slices,
                                                       const uint8_t* __restrict__ seq /* HS_SEQ_PAD readable bytes on both sides */, uint8_t* __restrict__ out) {
    const PolishSlice sl = slices[blockIdx.x];
    const PolishPiece pc = pieces[sl.piece];
    const int64_t a = ((int64_t)sl.window << 12) + ((int64_t)threadIdx.x << 4);   // the lane's 16-byte block of the output
    const int64_t o0 = pc.out_off, o1 = pc.out_off + pc.len;
    const int64_t lo = a > o0 ? a : o0, hi = a + 16 < o1 ? a + 16 : o1;
    if (lo >= hi) return;
    const int64_t i0 = a - o0;                                     // piece index of the block's first byte (-15 .. len - 1)
    // 16 source bytes in ascending address order: forward from src + i0, reverse the 16 bytes that end at src - i0
    const int64_t p = pc.rev ? pc.src - i0 - 15 : pc.src + i0;
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(seq + (p & ~(int64_t)3));
    const uint32_t sh = (uint32_t)(p & 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
    uint32_t d2 = __builtin_amdgcn_alignbyte(w3, w2, sh), d3 = __builtin_amdgcn_alignbyte(w4, w3, sh);
    uint4 v;
    if (pc.rev) {   // byte 3 of the last dword comes first; the complement of code c is 3 - c: the table read backwards
        const uint32_t t = 0x41434754u, x = 0x41414141u;   // "TGCA", "AAAA"
        v.x = polish_letters(__builtin_amdgcn_perm(0u, d3, 0x00010203u), t, x); v.y = polish_letters(__builtin_amdgcn_perm(0u, d2, 0x00010203u), t, x);
        v.z = polish_letters(__builtin_amdgcn_perm(0u, d1, 0x00010203u), t, x); v.w = polish_letters(__builtin_amdgcn_perm(0u, d0, 0x00010203u), t, x);
    } else {
        const uint32_t t = 0x54474341u, x = 0x54545454u;   // "ACGT", "TTTT"
        v.x = polish_letters(d0, t, x); v.y = polish_letters(d1, t, x); v.z = polish_letters(d2, t, x); v.w = polish_letters(d3, t, x);
    }
    if (hi - lo == 16) { *reinterpret_cast<uint4*>(out + a) = v; return; }
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (a + j >= lo && a + j < hi) out[a + j] = (uint8_t)(q[j >> 2] >> (8 * (j & 3)));
}

}  // namespace hsdev
