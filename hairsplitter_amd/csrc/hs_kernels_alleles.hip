// hs_kernels_alleles.hip -- which allele every group of reads carries at every SNP of its window: the crossing of the finished labels
// of stage 4 with the SNP columns of stage 3, on the device that holds both. The reference forms the same majority base per cluster and
// SNP inside merge_wrongly_split_haplotypes (separate_reads.cpp:1056-1113) and throws it away; here it is computed on the FINAL labels
// and returned. gfx950, wave64; plain vector stores only.
//
// A cell = (window, SNP column, group); groups = the distinct labels >= 0 of the window, ascending. The rule of a cell is stated once, in
// hs_alleles_host.h (allele_cell_finish), and both the host restatement and the kernel below end in it.
//
// Route of k_allele_cells: one workgroup per SNP column. Every entry of the column becomes a key (group slot << 8 | code), or the
// invalid key when its read has no label >= 0 in the window. The keys are sorted (block_bitonic_sort of hs_device.h, over the next power of two) and a
// lane per group finds its stretch of the sorted keys by bisection and hops from one run of equal keys to the next by bisection too.
// A per-group histogram over the 125 codes needs 250 B per group -- 300 groups do not fit the LDS next to anything else, 65535 not at
// all --, the sorted keys need 4 B per ENTRY whatever the number of groups, and a run costs log2(depth) probes however long it is.
//   depth <= HS_ALLELE_LDS_KEYS (2048): one wavefront, keys in LDS (k_allele_cells);
//   deeper columns (up to the path's 65535): queued by that kernel on a list, then sorted by 256 threads in a slab of global scratch
//   (k_allele_cells_wide, HS_ALLELE_WIDE_BLOCKS resident workgroups that walk the list; the launch is always queued, an empty list ends it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_alleles_host.h"
#include "hs_device.h"

#define HS_ALLELE_LDS_KEYS 2048         /* entries of a column whose keys one wavefront sorts in LDS (8 KB) */
#define HS_ALLELE_WIDE_KEYS 65536       /* keys of a slab of global scratch: the next power of two of the path's deepest column */
#define HS_ALLELE_WIDE_BLOCKS 64        /* workgroups (and slabs) of k_allele_cells_wide */

namespace hsdev {

struct AlleleCell { uint16_t n, best, second, n_ref, n_alt; uint8_t best_code, call; };      // == hs_allele_cell (12 bytes)

// the window of every SNP: the first window of its contig with win_start <= pos <= win_end (-1: none); has_snp[w] = 1 for every window that got one
__global__ __launch_bounds__(256) void k_allele_snp_window(const int32_t* __restrict__ snp_pos, const int32_t* __restrict__ snp_contig, int n_snps,
                                                           const int64_t* __restrict__ win_off, const int32_t* __restrict__ win_start,
                                                           const int32_t* __restrict__ win_end, int n_contigs, int32_t* __restrict__ snp_win,
                                                           int32_t* __restrict__ has_snp) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= n_snps) return;
    const int c = snp_contig[s], pos = snp_pos[s];
    int w = -1;
    if (c >= 0 && c < n_contigs) {
        // windows of a contig ascend: the first one whose end is not below pos
        long long lo = win_off[c], hi = win_off[c + 1];
        const long long end = hi;
        while (lo < hi) { const long long mid = (lo + hi) >> 1; if (win_end[mid] < pos) lo = mid + 1; else hi = mid; }
        if (lo < end && win_start[lo] <= pos) w = (int)lo;
    }
    snp_win[s] = w;
    if (w >= 0) has_snp[w] = 1;
}

// the groups of every window that has SNPs: its distinct labels >= 0, ascending, at grp_ids[label_off[w] ...] (room for one per read), their number
// in grp_n[w]. One workgroup per window; every round takes the smallest label above the last one taken (a window has a handful of groups;
// the rounds are exact for any ids and any number of them).
__global__ __launch_bounds__(256) void k_allele_groups(const int64_t* __restrict__ label_off, const int32_t* __restrict__ labels, int n_windows,
                                                       const int32_t* __restrict__ has_snp, int32_t* __restrict__ grp_n, int32_t* __restrict__ grp_ids) {
    __shared__ int32_t s_min[4];
    const int w = (int)blockIdx.x;
    if (w >= n_windows) return;
    if (!has_snp[w]) { if (threadIdx.x == 0) grp_n[w] = 0; return; }
    const long long l0 = label_off[w];
    const int n = (int)(label_off[w + 1] - l0);
    int32_t prev = -1;
    int count = 0;
    for (;;) {
        int32_t m = INT32_MAX;
        for (int i = (int)threadIdx.x; i < n; i += 256) { const int32_t v = labels[l0 + i]; if (v > prev && v < m) m = v; }
        for (int d = 32; d > 0; d >>= 1) m = min(m, __shfl_xor(m, d));
        if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = m;
        __syncthreads();
        m = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        __syncthreads();
        if (m == INT32_MAX || count >= n) break;      // (a label of INT32_MAX itself cannot be told from "none": ids are below it)
        if (threadIdx.x == 0) grp_ids[l0 + count] = m;
        ++count; prev = m;
    }
    if (threadIdx.x == 0) grp_n[w] = count;
}

// cells of every SNP (its window's groups; none without a window) and the SNP range of every window that has some
__global__ __launch_bounds__(256) void k_allele_cell_counts(const int32_t* __restrict__ snp_win, int n_snps, const int32_t* __restrict__ grp_n,
                                                            int32_t* __restrict__ n_cells, int32_t* __restrict__ win_snp_first, int32_t* __restrict__ win_snp_last) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= n_snps) return;
    const int w = snp_win[s];
    n_cells[s] = w >= 0 ? grp_n[w] : 0;
    if (w < 0) return;
    if (s == 0 || snp_win[s - 1] != w) win_snp_first[w] = s;
    if (s == n_snps - 1 || snp_win[s + 1] != w) win_snp_last[w] = s + 1;
}

// the group lists one after the other (grp_off: the scan of grp_n): what goes to the host
__global__ __launch_bounds__(256) void k_allele_pack_groups(const int32_t* __restrict__ grp_n, const int64_t* __restrict__ grp_off, const int64_t* __restrict__ label_off,
                                                            const int32_t* __restrict__ grp_ids, int n_windows, int32_t* __restrict__ grp_pack) {
    const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= n_windows) return;
    const int n = grp_n[w];
    const long long from = label_off[w], to = grp_off[w];
    for (int k = 0; k < n; ++k) grp_pack[to + k] = grp_ids[from + k];
}

// The column's keys -> its cells. `keys` (LDS or global scratch) has room for n_pow2 keys; every thread of the workgroup calls this.
static __device__ void allele_column(uint32_t* keys, int n_pow2, uint32_t* s_calls /* [8] in LDS */, long long e0, int depth,
                                     const int32_t* __restrict__ col_idx, const uint8_t* __restrict__ col_code, const int32_t* __restrict__ win_labels,
                                     int n_reads, const int32_t* __restrict__ grp, int G, uint8_t ref, uint8_t alt, AlleleCell* __restrict__ out,
                                     int32_t* __restrict__ n_calls_out) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    if (tid < 8) s_calls[tid] = 0;
    for (int i = tid; i < n_pow2; i += nt) {
        uint32_t key = 0xFFFFFFFFu;
        if (i < depth) {
            const int r = col_idx[e0 + i];
            const int32_t lab = (r >= 0 && r < n_reads) ? win_labels[r] : -2;      // a read the window does not know has no label
            if (lab >= 0) {
                int lo = 0, hi = G;      // the label is one of the window's groups: its slot
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (grp[mid] < lab) lo = mid + 1; else hi = mid; }
                if (lo < G && grp[lo] == lab) key = ((uint32_t)lo << 8) | col_code[e0 + i];
            }
        }
        keys[i] = key;
    }
    __syncthreads();
    block_bitonic_sort(keys, n_pow2);
    // first index whose key is >= v
    auto lower = [&](uint32_t v, int from) { int lo = from, hi = depth; while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < v) lo = mid + 1; else hi = mid; } return lo; };
    for (int g = tid; g < G; g += nt) {
        const int a = lower((uint32_t)g << 8, 0), b = lower(((uint32_t)g + 1) << 8, a);
        hs::AlleleCounts ac;
        for (int i = a; i < b;) {
            const uint32_t key = keys[i];
            const int nx = lower(key + 1, i + 1);      // (key + 1 <= (g + 1) << 8: no overflow below the invalid key)
            ac.add_run((uint8_t)(key & 255u), (uint32_t)(nx - i), ref, alt);
            i = nx;
        }
        const hs::AlleleCellValue v = hs::allele_cell_finish(ac);
        AlleleCell c;
        c.n = (uint16_t)v.n; c.best = (uint16_t)v.best; c.second = (uint16_t)v.second; c.n_ref = (uint16_t)v.n_ref; c.n_alt = (uint16_t)v.n_alt;
        c.best_code = v.best_code; c.call = v.call;
        out[g] = c;
        if (v.call) atomicOr(&s_calls[v.call >> 5], 1u << (v.call & 31));
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < 8; ++k) n += __popc(s_calls[k]);
        *n_calls_out = n;
    }
    __syncthreads();
}

// what the column kernels of this table and of the recruit table (hs_kernels_recruit.hip) read: the columns, the dense labels and the plan
struct ColumnArgs {
    const int64_t* col_off; const int32_t* col_idx; const uint8_t* col_code; int n_snps;
    const int32_t* snp_win; const int64_t* label_off; const int32_t* labels; long long n_labels; int n_windows;
    const int32_t* grp_n; const int32_t* grp_ids; const int64_t* cell_off; long long cells_cap;
};
// a column as those kernels see it: its window and the window's G groups, its `depth` entries from e0 (the path's columns hold at most
// 65535; the C ABI refuses deeper ones), the window's n_reads labels from l0. false: nothing to do -- no window (then depth = 0), no
// group, or labels that are not the call's
struct Column { int w, G, depth; long long e0, l0, n_reads; };
static __device__ __forceinline__ bool column_load(const ColumnArgs& A, int s, Column& c) {
    c.w = A.snp_win[s]; c.G = 0; c.depth = 0;
    if (c.w < 0 || c.w >= A.n_windows) return false;
    c.G = A.grp_n[c.w];
    c.e0 = A.col_off[s];
    const long long d = A.col_off[s + 1] - c.e0;
    c.depth = d < 0 ? 0 : (d > 65535 ? 65535 : (int)d);
    c.l0 = A.label_off[c.w];
    c.n_reads = A.label_off[c.w + 1] - c.l0;
    return c.G > 0 && c.l0 >= 0 && c.l0 + c.n_reads <= A.n_labels;
}

struct AlleleArgs : ColumnArgs {
    const uint8_t* snp_ref; const uint8_t* snp_alt; AlleleCell* cells; int32_t* n_calls;
    int32_t* wide_count; int32_t* wide_list;      // columns deeper than HS_ALLELE_LDS_KEYS, for k_allele_cells_wide
};

// one column, by whichever kernel owns it; false: the column is not this route's (too deep for `cap` keys)
static __device__ bool allele_one(const AlleleArgs& A, int s, uint32_t* keys, int cap, uint32_t* s_calls) {
    Column c;
    const bool work = column_load(A, s, c);
    if (c.depth > cap) return false;
    if (!work) { if (threadIdx.x == 0) A.n_calls[s] = 0; return true; }
    const long long c0 = A.cell_off[s];
    if (c0 < 0 || c0 + c.G > A.cells_cap) { if (threadIdx.x == 0) A.n_calls[s] = -1; return true; }      // never write beyond the caller's cells
    allele_column(keys, pow2_at_least(c.depth), s_calls, c.e0, c.depth, A.col_idx, A.col_code, A.labels + c.l0, (int)c.n_reads, A.grp_ids + c.l0, c.G,
                  A.snp_ref[s], A.snp_alt[s], A.cells + c0, A.n_calls + s);
    return true;
}

__global__ __launch_bounds__(64) void k_allele_cells(AlleleArgs A) {
    __shared__ uint32_t s_keys[HS_ALLELE_LDS_KEYS];
    __shared__ uint32_t s_calls[8];
    const int s = (int)blockIdx.x;
    if (s >= A.n_snps) return;
    if (!allele_one(A, s, s_keys, HS_ALLELE_LDS_KEYS, s_calls) && threadIdx.x == 0) wide_list_push(A.wide_count, A.wide_list, A.n_snps, s);
}

__global__ __launch_bounds__(256) void k_allele_cells_wide(AlleleArgs A, uint32_t* __restrict__ slabs) {
    __shared__ uint32_t s_calls[8];
    const int n = *A.wide_count;
    uint32_t* keys = slabs + (size_t)blockIdx.x * HS_ALLELE_WIDE_KEYS;
    for (int i = (int)blockIdx.x; i < n && i < A.n_snps; i += (int)gridDim.x) (void)allele_one(A, A.wide_list[i], keys, HS_ALLELE_WIDE_KEYS, s_calls);
}

// sparse labels (per window: ascending read ids and their labels, everybody else -2) -> the dense form the kernels above read
__global__ __launch_bounds__(256) void k_allele_fill_absent(int32_t* __restrict__ labels, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) labels[i] = -2;
}
__global__ __launch_bounds__(256) void k_allele_scatter_labels(const int64_t* __restrict__ row_off, const int32_t* __restrict__ ids, const int32_t* __restrict__ lab,
                                                               const int64_t* __restrict__ label_off, int n_windows, int32_t* __restrict__ labels) {
    const int w = (int)blockIdx.x;
    if (w >= n_windows) return;
    const long long l0 = label_off[w];
    const int n = (int)(label_off[w + 1] - l0);
    for (long long e = row_off[w] + threadIdx.x; e < row_off[w + 1]; e += 256) { const int r = ids[e]; if (r >= 0 && r < n) labels[l0 + r] = lab[e]; }
}

}  // namespace hsdev
