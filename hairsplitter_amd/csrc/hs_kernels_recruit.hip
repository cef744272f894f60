// hs_kernels_recruit.hip -- which group of its window a read without a label belongs to: the SNP columns crossed with the calls of the allele
// table (hs_kernels_alleles.hip) for the reads stage 4 left at -2 (not at both ends of the window, separate_reads.cpp:1590-1622) or -1 (a
// cluster below the size filter, separate_reads.cpp:938). gfx950, wave64; plain vector stores and no-return integer atomics only.
//
// A row = (window, read) with at least one entry in a column of the window and a label selected by `which`. The rule of a row is stated
// once, in hs_recruit_host.h (recruit_selected, recruit_entry, RecruitChoice, recruit_row), and the kernels below end in it.
//   k_recruit_mark      one wavefront per SNP column, lanes = entries in rounds of 64: the read's slot of the dense label layout gets
//                       flag = 1 and its number of counter words (1 + 2 G); both stores are idempotent. Two scans (k_scan_*) turn them into the row index and
//                       the counter offset of every slot: rows come out window-major, reads ascending.
//   k_recruit_count     one wavefront per column, behind the cells: per group the call of the column's cell is one wave-uniform load,
//                       every flagged entry lane adds to m or x of its (row, group) and once to the row's n_entries. Integer sums: any order.
//   k_recruit_decide    one lane per slot for windows of up to 64 groups; k_recruit_decide_wide one wavefront per row beyond that
//                       (lanes = groups, the choices merged across the wave). Both write the 40-byte row record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_recruit_host.h"

#define HS_RECRUIT_LANE_GROUPS 64      /* windows of up to this many groups are decided by one lane per row */

namespace hsdev {

struct RecruitArgs : ColumnArgs {      // (ColumnArgs, Column, column_load: hs_kernels_alleles.hip)
    const AlleleCell* cells;
    int32_t* flag; int32_t* ctr_n; const int64_t* row_idx; const int64_t* ctr_off;
    uint32_t* counters; long long counters_cap; hs_recruit_row* rows; long long rows_cap; int64_t* win_row_off; int32_t* status;
    hs_recruit_params params;
};

__global__ __launch_bounds__(64) void k_recruit_mark(RecruitArgs A) {
    const int s = (int)blockIdx.x;
    Column c;
    if (s >= A.n_snps || !column_load(A, s, c)) return;      // (a window with SNPs and no group has no rows)
    for (int i = (int)threadIdx.x; i < c.depth; i += 64) {
        const int r = A.col_idx[c.e0 + i];
        if (r < 0 || r >= c.n_reads) continue;
        if (!hs::recruit_selected(A.labels[c.l0 + r], A.params.which)) continue;
        A.flag[c.l0 + r] = 1;
        A.ctr_n[c.l0 + r] = 1 + 2 * c.G;
    }
}

// rows of every window: the row index at the window's first slot
__global__ __launch_bounds__(256) void k_recruit_win_rows(RecruitArgs A) {
    const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w > A.n_windows) return;
    long long l = A.label_off[w];
    l = l < 0 ? 0 : (l > A.n_labels ? A.n_labels : l);
    A.win_row_off[w] = A.row_idx[l];
    if (w == 0) *A.status = (A.row_idx[A.n_labels] > A.rows_cap || A.ctr_off[A.n_labels] > A.counters_cap) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_recruit_count(RecruitArgs A) {
    const int s = (int)blockIdx.x;
    Column c;
    if (s >= A.n_snps || !column_load(A, s, c)) return;
    const int G = c.G, depth = c.depth;
    const long long e0 = c.e0, l0 = c.l0, n_reads = c.n_reads, c0 = A.cell_off[s];
    if (c0 < 0 || c0 + G > A.cells_cap) return;      // (the cell kernel refused the column too: n_calls = -1 stops the assembly)
    const AlleleCell* __restrict__ cells = A.cells + c0;
    for (int base = 0; base < depth; base += 64) {
        const int i = base + (int)threadIdx.x;
        long long at = -1;
        uint8_t code = 0;
        if (i < depth) {
            const int r = A.col_idx[e0 + i];
            if (r >= 0 && r < n_reads && A.flag[l0 + r]) {
                const long long o = A.ctr_off[l0 + r];
                if (o >= 0 && o + 1 + 2 * (long long)G <= A.counters_cap) { at = o; code = A.col_code[e0 + i]; }
            }
        }
        if (__ballot(at >= 0) == 0) continue;      // (no row among these 64 entries: wave-uniform)
        if (at >= 0) atomicAdd(A.counters + at, 1u);
        for (int k = 0; k < G; ++k) {
            const uint8_t call = cells[k].call;      // (the same address in every lane)
            const int what = hs::recruit_entry(code, call);
            if (at >= 0 && what) atomicAdd(A.counters + at + 1 + 2 * k + (what - 1), 1u);
        }
    }
}

// the window of a slot of the dense label layout: the last one that begins at or before it (windows without reads share their offset with the next)
static __device__ __forceinline__ int recruit_window_of(const int64_t* __restrict__ label_off, int n_windows, long long slot) {
    int lo = 0, hi = n_windows;      // first w with label_off[w] > slot
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (label_off[mid] <= slot) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

__global__ __launch_bounds__(256) void k_recruit_decide(RecruitArgs A) {
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= A.n_labels || !A.flag[slot]) return;
    const int w = recruit_window_of(A.label_off, A.n_windows, slot);
    if (w < 0) return;
    const int G = A.grp_n[w];
    if (G <= 0 || G > HS_RECRUIT_LANE_GROUPS) return;
    const long long row = A.row_idx[slot], at = A.ctr_off[slot];
    if (row < 0 || row >= A.rows_cap || at < 0 || at + 1 + 2 * (long long)G > A.counters_cap) return;
    const long long l0 = A.label_off[w];
    hs::RecruitChoice c;
    for (int k = 0; k < G; ++k) c.offer(k, A.counters[at + 1 + 2 * k], A.counters[at + 2 + 2 * k]);
    A.rows[row] = hs::recruit_row(A.params, (int32_t)(slot - l0), A.labels[slot], G, A.grp_ids + l0, c, A.counters[at]);
}

__global__ __launch_bounds__(256) void k_recruit_decide_wide(RecruitArgs A) {
    const int w = (int)blockIdx.x;
    if (w >= A.n_windows) return;
    const int G = A.grp_n[w];
    if (G <= HS_RECRUIT_LANE_GROUPS) return;
    const long long l0 = A.label_off[w];
    const long long n_reads = A.label_off[w + 1] - l0;
    if (l0 < 0 || l0 + n_reads > A.n_labels) return;
    const int lane = (int)threadIdx.x & 63;
    for (long long r = threadIdx.x >> 6; r < n_reads; r += 4) {      // (wave-uniform: every lane of a wavefront walks the same reads)
        const long long slot = l0 + r;
        if (!A.flag[slot]) continue;
        const long long row = A.row_idx[slot], at = A.ctr_off[slot];
        if (row < 0 || row >= A.rows_cap || at < 0 || at + 1 + 2 * (long long)G > A.counters_cap) continue;
        hs::RecruitChoice c;
        for (int k = lane; k < G; k += 64) c.offer(k, A.counters[at + 1 + 2 * k], A.counters[at + 2 + 2 * k]);
        for (int d = 32; d > 0; d >>= 1) {
            hs::RecruitChoice o;
            o.best = __shfl_xor(c.best, d); o.m_best = __shfl_xor(c.m_best, d); o.x_best = __shfl_xor(c.x_best, d);
            o.second = __shfl_xor(c.second, d); o.m_second = __shfl_xor(c.m_second, d); o.x_second = __shfl_xor(c.x_second, d);
            c.merge(o);
        }
        if (lane == 0) A.rows[row] = hs::recruit_row(A.params, (int32_t)r, A.labels[slot], G, A.grp_ids + l0, c, A.counters[at]);
    }
}

}  // namespace hsdev
