// hs_capi_recruit.inc -- part of hs_capi.hip: the recruit table (include/hairsplitter_hip.h: hs_group_recruit, hs_recruit_reads, and the share of
// a contig group of a pipeline). Kernels in hs_kernels_recruit.hip, the host side of the table in hs_recruit_host.cpp. The stage-level route is
// alleles_on_device of hs_capi_alleles.inc with thresholds: it queues the two launchers below between its own and adds no host wait.
static_assert(sizeof(hs_recruit_row) == 40, "hs_recruit_row layout");

namespace {

// the parts of d_work (hs_recruit_layout) behind the allele plan's: flag and ctr_n [n_labels] back to back (one clearing), the two
// scans' outputs [n_labels + 1], win_row_off [W + 1], status; `internal`: ctr_n and the scans' tile sums and offsets
static RecruitWork recruit_work(int32_t S, int32_t W, int64_t n_labels) {
    RecruitWork r;
    r.a = allele_work(S, W, n_labels);
    r.L.alleles = r.a.L;
    WorkParts p{r.a.L.total_bytes};
    r.L.flag = p.take(n_labels * 4);
    r.L.internal = p.o;
    r.ctr_n = p.take(n_labels * 4);
    r.L.row_idx = p.take((n_labels + 1) * 8); r.L.ctr_off = p.take((n_labels + 1) * 8);
    r.L.win_row_off = p.take(((int64_t)W + 1) * 8); r.L.status = p.take(4);
    r.tile_sum = p.take((int64_t)std::max(scan_tiles(n_labels), 1) * 16);
    r.L.total_bytes = p.o;
    return r;
}

static hsdev::RecruitArgs recruit_args(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params) {
    hsdev::RecruitArgs A{};      // (no cells, counters or rows: the second step adds its own)
    column_args(in, work, rw.a, 0, A);
    A.flag = (int32_t*)(work + rw.L.flag); A.ctr_n = (int32_t*)(work + rw.ctr_n);
    A.row_idx = (const int64_t*)(work + rw.L.row_idx); A.ctr_off = (const int64_t*)(work + rw.L.ctr_off);
    A.win_row_off = (int64_t*)(work + rw.L.win_row_off); A.status = (int32_t*)(work + rw.L.status);
    A.params = params;
    return A;
}
static bool recruit_nothing(const AlleleDevIn& in) { return in.n_snps == 0 || in.n_windows == 0 || in.n_labels == 0; }

// behind the allele plan: the flag of every row's slot, then row index and counter offset of every slot
static int recruit_plan_launch(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params, hipStream_t st) {
    const long long n = in.n_labels;
    if (recruit_nothing(in)) {      // no rows: the two totals the host reads
        HS_HIP(hipMemsetAsync(work + rw.L.row_idx + n * 8, 0, 8, st));
        HS_HIP(hipMemsetAsync(work + rw.L.ctr_off + n * 8, 0, 8, st));
        return HS_OK;
    }
    const hsdev::RecruitArgs A = recruit_args(in, work, rw, params);
    HS_HIP(hipMemsetAsync(A.flag, 0, (size_t)(rw.ctr_n - rw.L.flag) + (size_t)n * 4, st));
    hipLaunchKernelGGL(hsdev::k_recruit_mark, dim3((unsigned)in.n_snps), dim3(64), 0, st, A);
    long long* tile_sum = (long long*)(work + rw.tile_sum);
    if (int rc = exclusive_scan_launch(A.flag, (int)n, (int64_t*)(work + rw.L.row_idx), tile_sum, st)) return rc;
    return exclusive_scan_launch(A.ctr_n, (int)n, (int64_t*)(work + rw.L.ctr_off), tile_sum, st);      // (it takes the tile scratch over: the stream orders it behind the first)
}

// behind the cells: counters, then the rows of the plan in `work`
static int recruit_rows_launch(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params, const hs_allele_cell* d_cells, int64_t cells_cap,
                               uint32_t* d_counters, int64_t counters_cap, hs_recruit_row* d_rows, int64_t rows_cap, hipStream_t st) {
    const int W = in.n_windows;
    if (recruit_nothing(in)) {
        HS_HIP(hipMemsetAsync(work + rw.L.win_row_off, 0, ((size_t)W + 1) * 8, st));
        HS_HIP(hipMemsetAsync(work + rw.L.status, 0, 4, st));
        return HS_OK;
    }
    hsdev::RecruitArgs A = recruit_args(in, work, rw, params);
    A.cells = reinterpret_cast<const hsdev::AlleleCell*>(d_cells); A.cells_cap = cells_cap; A.counters = d_counters; A.counters_cap = d_counters ? counters_cap : 0;
    A.rows = d_rows; A.rows_cap = d_rows ? rows_cap : 0;
    if (A.counters_cap > 0) HS_HIP(hipMemsetAsync(d_counters, 0, (size_t)A.counters_cap * 4, st));
    hipLaunchKernelGGL(hsdev::k_recruit_win_rows, dim3((unsigned)(W / 256 + 1)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_recruit_count, dim3((unsigned)in.n_snps), dim3(64), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_recruit_decide, dim3((unsigned)((in.n_labels + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_recruit_decide_wide, dim3((unsigned)W), dim3(256), 0, st, A);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

}  // namespace

extern "C" {

int hs_group_recruit_layout(int32_t n_snps, int32_t n_windows, int64_t n_labels, hs_recruit_layout* out) {
    if (!out || n_snps < 0 || n_windows < 0 || n_labels < 0 || n_labels > 0x7fffffff - HS_SCAN_TILE) { set_error("hs_group_recruit_layout: bad arguments"); return HS_EINVAL; }
    *out = recruit_work(n_snps, n_windows, n_labels).L;
    return HS_OK;
}

int hs_group_recruit(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const uint8_t* d_snp_ref, const uint8_t* d_snp_alt,
                     const int32_t* d_snp_pos, const int32_t* d_snp_contig, int32_t n_snps, const int64_t* d_win_off, const int32_t* d_win_start,
                     const int32_t* d_win_end, int32_t n_contigs, int32_t n_windows, const int64_t* d_label_off, const int32_t* d_labels, int64_t n_labels,
                     const hs_recruit_params* params, void* d_work, hs_allele_cell* d_cells, int64_t cells_cap, uint32_t* d_counters, int64_t counters_cap,
                     hs_recruit_row* d_rows, int64_t rows_cap, void* stream) {
    if (int rc = require_device()) return rc;
    if (n_snps < 0 || n_windows < 0 || n_contigs < 0 || n_labels < 0 || n_labels > 0x7fffffff - HS_SCAN_TILE || !d_work || (d_cells && (cells_cap < 0 || counters_cap < 0 || rows_cap < 0))) {
        set_error("hs_group_recruit: bad arguments"); return HS_EINVAL;
    }
    const hs_recruit_params prm = params ? *params : hs_recruit_params_default();
    if (!hs::recruit_params_valid(prm)) { set_error("hs_group_recruit: thresholds out of range"); return HS_EINVAL; }
    const RecruitWork rw = recruit_work(n_snps, n_windows, n_labels);
    const AlleleDevIn in{d_col_off, d_col_idx, d_col_code, d_snp_ref, d_snp_alt, d_snp_pos, d_snp_contig, n_snps, d_win_off, d_win_start, d_win_end,
                         n_contigs, n_windows, d_label_off, d_labels, n_labels};
    hipStream_t st = (hipStream_t)stream;
    if (!d_cells) {
        if (int rc = allele_plan_launch(in, (char*)d_work, rw.a, st)) return rc;
        return recruit_plan_launch(in, (char*)d_work, rw, prm, st);
    }
    if (int rc = allele_cells_launch(in, (char*)d_work, rw.a, d_cells, cells_cap, st)) return rc;
    return recruit_rows_launch(in, (char*)d_work, rw, prm, d_cells, cells_cap, d_counters, counters_cap, d_rows, rows_cap, st);
}

int hs_recruit_reads(const hs_sr_contig* contigs, int32_t n_contigs, const hs_sr_result* sr, const hs_recruit_params* params, hs_allele_table** alleles,
                     hs_recruit_table** out) {
    if (!out) { set_error("hs_recruit_reads: null argument"); return HS_EINVAL; }
    *out = nullptr;
    if (alleles) *alleles = nullptr;
    const hs_recruit_params prm = params ? *params : hs_recruit_params_default();
    if (!hs::recruit_params_valid(prm)) { set_error("hs_recruit_reads: thresholds out of range"); return HS_EINVAL; }
    hs_allele_table* at = nullptr;
    if (int rc = haplotype_tables(contigs, n_contigs, sr, &at, &prm, out)) return rc;
    if (alleles) *alleles = at; else hs::alleles_free(at);
    return HS_OK;
}

}  // extern "C"
