// hs_capi_recruit.inc -- part of hs_capi.hip: the recruit table (include/hairsplitter_hip.h: hs_group_recruit, hs_recruit_reads, and the share of
// a contig group of a pipeline). Kernels in hs_kernels_recruit.hip, the host side of the table in hs_recruit_host.cpp. The stage-level route is
// alleles_on_device of hs_capi_alleles.inc with a RecruitReq: it queues the two launchers below between its own and adds no host wait.
static_assert(sizeof(hs_recruit_row) == 40, "hs_recruit_row layout");

namespace {

// the parts of d_work (hs_recruit_layout), 256-byte aligned, behind the allele plan's: flag and ctr_n [n_labels] back to back (one clearing), the two
// scans' outputs [n_labels + 1], win_row_off [W + 1], status; `internal`: ctr_n and the scans' tile sums and offsets
static RecruitWork recruit_work(int32_t S, int32_t W, int64_t n_labels) {
    RecruitWork r;
    r.a = allele_work(S, W, n_labels);
    r.L.alleles = r.a.L;
    int64_t o = r.a.L.total_bytes;
    auto take = [&](int64_t bytes) { const int64_t at = o; o = (o + std::max<int64_t>(bytes, 4) + 255) & ~(int64_t)255; return at; };
    r.n_tiles = (int)((n_labels + HS_SCAN_TILE - 1) / HS_SCAN_TILE);
    r.L.flag = take(n_labels * 4);
    r.L.internal = o;
    r.ctr_n = take(n_labels * 4);
    r.L.row_idx = take((n_labels + 1) * 8); r.L.ctr_off = take((n_labels + 1) * 8);
    r.L.win_row_off = take(((int64_t)W + 1) * 8); r.L.status = take(4);
    r.tile_sum = take((int64_t)std::max(r.n_tiles, 1) * 16);
    r.L.total_bytes = o;
    return r;
}

static hsdev::RecruitArgs recruit_args(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params) {
    hsdev::RecruitArgs A;
    A.col_off = in.d_col_off; A.col_idx = in.d_col_idx; A.col_code = in.d_col_code; A.n_snps = in.n_snps;
    A.snp_win = (const int32_t*)(work + rw.a.L.snp_win); A.label_off = in.d_label_off; A.labels = in.d_labels; A.n_labels = in.n_labels; A.n_windows = in.n_windows;
    A.grp_n = (const int32_t*)(work + rw.a.L.grp_n); A.grp_ids = (const int32_t*)(work + rw.a.L.grp_ids); A.cell_off = (const int64_t*)(work + rw.a.L.cell_off);
    A.cells = nullptr; A.cells_cap = 0;
    A.flag = (int32_t*)(work + rw.L.flag); A.ctr_n = (int32_t*)(work + rw.ctr_n);
    A.row_idx = (const int64_t*)(work + rw.L.row_idx); A.ctr_off = (const int64_t*)(work + rw.L.ctr_off);
    A.counters = nullptr; A.counters_cap = 0; A.rows = nullptr; A.rows_cap = 0;
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
    int64_t* row_idx = (int64_t*)(work + rw.L.row_idx); int64_t* ctr_off = (int64_t*)(work + rw.L.ctr_off);
    hipLaunchKernelGGL(hsdev::k_scan_tile_sums, dim3((unsigned)rw.n_tiles), dim3(256), 0, st, A.flag, (int)n, tile_sum);
    hipLaunchKernelGGL(hsdev::k_scan_tile_offsets, dim3(1), dim3(1024), 0, st, tile_sum, rw.n_tiles, tile_sum + rw.n_tiles, row_idx + n);
    hipLaunchKernelGGL(hsdev::k_scan_apply, dim3((unsigned)rw.n_tiles), dim3(256), 0, st, A.flag, (int)n, tile_sum + rw.n_tiles, row_idx);
    // (the second scan takes the tile scratch over: the stream orders it behind the first)
    hipLaunchKernelGGL(hsdev::k_scan_tile_sums, dim3((unsigned)rw.n_tiles), dim3(256), 0, st, A.ctr_n, (int)n, tile_sum);
    hipLaunchKernelGGL(hsdev::k_scan_tile_offsets, dim3(1), dim3(1024), 0, st, tile_sum, rw.n_tiles, tile_sum + rw.n_tiles, ctr_off + n);
    hipLaunchKernelGGL(hsdev::k_scan_apply, dim3((unsigned)rw.n_tiles), dim3(256), 0, st, A.ctr_n, (int)n, tile_sum + rw.n_tiles, ctr_off);
    HS_HIP(hipGetLastError());
    return HS_OK;
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
    A.cells = (const uint8_t*)d_cells; A.cells_cap = cells_cap; A.counters = d_counters; A.counters_cap = d_counters ? counters_cap : 0;
    A.rows = d_rows; A.rows_cap = d_rows ? rows_cap : 0;
    if (A.counters_cap > 0) HS_HIP(hipMemsetAsync(d_counters, 0, (size_t)A.counters_cap * 4, st));
    hipLaunchKernelGGL(hsdev::k_recruit_win_rows, dim3((unsigned)(W / 256 + 1)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_recruit_count, dim3((unsigned)in.n_snps), dim3(64), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_recruit_decide, dim3((unsigned)((in.n_labels + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_recruit_decide_wide, dim3((unsigned)W), dim3(256), 0, st, A);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// the share of one contig group of a pipeline: pipeline_group_alleles with a RecruitReq
static int pipeline_group_recruit(const hs_sr_result* r, const hs::SrSparseLabels& sp, const hs_cv_result* cv, float rsa, int c0, HipSrOps& ops, const hs_recruit_params& params,
                                  hs_allele_table** alleles, hs_recruit_table** out) {
    RecruitReq rq;
    rq.params = params;
    if (int rc = pipeline_group_alleles(r, sp, cv, rsa, c0, ops, alleles, &rq)) return rc;
    *out = rq.table;
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
    RecruitReq rq;
    rq.params = params ? *params : hs_recruit_params_default();
    if (!hs::recruit_params_valid(rq.params)) { set_error("hs_recruit_reads: thresholds out of range"); return HS_EINVAL; }
    hs_allele_table* at = nullptr;
    if (int rc = haplotype_tables(contigs, n_contigs, sr, &at, &rq)) return rc;
    if (alleles) *alleles = at; else hs::alleles_free(at);
    *out = rq.table;
    return HS_OK;
}

}  // extern "C"
