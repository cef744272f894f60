// hs_capi_alleles.inc -- part of hs_capi.hip: the allele table (include/hairsplitter_hip.h: hs_group_alleles, hs_haplotype_alleles, and the
// share of a contig group of a pipeline). Kernels in hs_kernels_alleles.hip, the host side of the table in hs_alleles_host.cpp.
static_assert(sizeof(hs_allele_cell) == sizeof(hsdev::AlleleCell) && sizeof(hs_allele_cell) == 12, "hs_allele_cell layout");

namespace {

// the parts of d_work (hs_allele_layout), 256-byte aligned. The small arrays lie in front (they go to the host in one shipment), then the
// group lists per window (room for one group per read) and one after the other; `internal`: has_snp [W], n_cells [S], the scans' tile sums
// and offsets, the wide route's counter and list [S], then its slabs
struct AlleleWork {
    hs_allele_layout L;
    int64_t has_snp, n_cells, tile_sum, wide_count, wide_list, slabs;
    int n_tiles, n_tiles_w;
};
static AlleleWork allele_work(int32_t S, int32_t W, int64_t n_labels) {
    AlleleWork a;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o = (o + std::max<int64_t>(bytes, 4) + 255) & ~(int64_t)255; return at; };
    a.n_tiles = (S + HS_SCAN_TILE - 1) / HS_SCAN_TILE; a.n_tiles_w = (W + HS_SCAN_TILE - 1) / HS_SCAN_TILE;
    a.L.snp_win = take((int64_t)S * 4); a.L.grp_n = take((int64_t)W * 4);
    a.L.win_snp_first = take((int64_t)W * 4); a.L.win_snp_last = take((int64_t)W * 4);      // (the two lie back to back: one clearing)
    a.L.cell_off = take(((int64_t)S + 1) * 8); a.L.grp_off = take(((int64_t)W + 1) * 8); a.L.n_calls = take((int64_t)S * 4);
    a.L.grp_ids = take(n_labels * 4); a.L.grp_pack = take(n_labels * 4);
    a.L.internal = o;
    a.has_snp = take((int64_t)W * 4); a.n_cells = take((int64_t)S * 4); a.tile_sum = take((int64_t)std::max(std::max(a.n_tiles, a.n_tiles_w), 1) * 16);
    a.wide_count = take(4); a.wide_list = take((int64_t)S * 4);
    a.slabs = take((int64_t)HS_ALLELE_WIDE_BLOCKS * HS_ALLELE_WIDE_KEYS * 4);
    a.L.total_bytes = o;
    return a;
}

struct AlleleDevIn {
    const int64_t* d_col_off; const int32_t* d_col_idx; const uint8_t* d_col_code;
    const uint8_t* d_snp_ref; const uint8_t* d_snp_alt; const int32_t* d_snp_pos; const int32_t* d_snp_contig; int32_t n_snps;
    const int64_t* d_win_off; const int32_t* d_win_start; const int32_t* d_win_end; int32_t n_contigs, n_windows;
    const int64_t* d_label_off; const int32_t* d_labels; int64_t n_labels;
};

// the plan: window of every SNP, groups of every window that has SNPs, SNP ranges, cell offsets
static int allele_plan_launch(const AlleleDevIn& in, char* work, const AlleleWork& a, hipStream_t st) {
    const int S = in.n_snps, W = in.n_windows;
    int32_t* snp_win = (int32_t*)(work + a.L.snp_win); int32_t* grp_n = (int32_t*)(work + a.L.grp_n); int32_t* grp_ids = (int32_t*)(work + a.L.grp_ids);
    int32_t* first = (int32_t*)(work + a.L.win_snp_first); int32_t* last = (int32_t*)(work + a.L.win_snp_last);
    int64_t* cell_off = (int64_t*)(work + a.L.cell_off); int64_t* grp_off = (int64_t*)(work + a.L.grp_off); int32_t* grp_pack = (int32_t*)(work + a.L.grp_pack);
    int32_t* has_snp = (int32_t*)(work + a.has_snp); int32_t* n_cells = (int32_t*)(work + a.n_cells);
    long long* tile_sum = (long long*)(work + a.tile_sum);
    HS_HIP(hipMemsetAsync(first, 0, (size_t)(a.L.win_snp_last - a.L.win_snp_first) + (size_t)std::max(W, 1) * 4, st));
    HS_HIP(hipMemsetAsync(has_snp, 0, (size_t)std::max(W, 1) * 4, st));
    if (S == 0 || W == 0) {
        if (W) HS_HIP(hipMemsetAsync(grp_n, 0, (size_t)W * 4, st));
        if (S) HS_HIP(hipMemsetAsync(snp_win, 0xFF, (size_t)S * 4, st));
        HS_HIP(hipMemsetAsync(cell_off, 0, ((size_t)S + 1) * 8, st));
        HS_HIP(hipMemsetAsync(grp_off, 0, ((size_t)W + 1) * 8, st));
        return HS_OK;
    }
    hipLaunchKernelGGL(hsdev::k_allele_snp_window, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, in.d_snp_pos, in.d_snp_contig, S, in.d_win_off,
                       in.d_win_start, in.d_win_end, in.n_contigs, snp_win, has_snp);
    hipLaunchKernelGGL(hsdev::k_allele_groups, dim3((unsigned)W), dim3(256), 0, st, in.d_label_off, in.d_labels, W, has_snp, grp_n, grp_ids);
    hipLaunchKernelGGL(hsdev::k_allele_cell_counts, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, snp_win, S, grp_n, n_cells, first, last);
    hipLaunchKernelGGL(hsdev::k_scan_tile_sums, dim3((unsigned)a.n_tiles), dim3(256), 0, st, n_cells, S, tile_sum);
    hipLaunchKernelGGL(hsdev::k_scan_tile_offsets, dim3(1), dim3(1024), 0, st, tile_sum, a.n_tiles, tile_sum + a.n_tiles, cell_off + S);
    hipLaunchKernelGGL(hsdev::k_scan_apply, dim3((unsigned)a.n_tiles), dim3(256), 0, st, n_cells, S, tile_sum + a.n_tiles, cell_off);
    // (the second scan takes the tile scratch over: the stream orders it behind the first)
    hipLaunchKernelGGL(hsdev::k_scan_tile_sums, dim3((unsigned)a.n_tiles_w), dim3(256), 0, st, grp_n, W, tile_sum);
    hipLaunchKernelGGL(hsdev::k_scan_tile_offsets, dim3(1), dim3(1024), 0, st, tile_sum, a.n_tiles_w, tile_sum + a.n_tiles_w, grp_off + W);
    hipLaunchKernelGGL(hsdev::k_scan_apply, dim3((unsigned)a.n_tiles_w), dim3(256), 0, st, grp_n, W, tile_sum + a.n_tiles_w, grp_off);
    hipLaunchKernelGGL(hsdev::k_allele_pack_groups, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, grp_n, grp_off, in.d_label_off, grp_ids, W, grp_pack);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// the cells of the plan in `work`
static int allele_cells_launch(const AlleleDevIn& in, char* work, const AlleleWork& a, hs_allele_cell* d_cells, int64_t cells_cap, hipStream_t st) {
    const int S = in.n_snps;
    if (S == 0) return HS_OK;
    if (in.n_windows == 0) { HS_HIP(hipMemsetAsync(work + a.L.n_calls, 0, (size_t)S * 4, st)); return HS_OK; }
    hsdev::AlleleArgs A;
    A.col_off = in.d_col_off; A.col_idx = in.d_col_idx; A.col_code = in.d_col_code; A.snp_ref = in.d_snp_ref; A.snp_alt = in.d_snp_alt;
    A.snp_win = (const int32_t*)(work + a.L.snp_win); A.label_off = in.d_label_off; A.labels = in.d_labels;
    A.grp_n = (const int32_t*)(work + a.L.grp_n); A.grp_ids = (const int32_t*)(work + a.L.grp_ids); A.cell_off = (const int64_t*)(work + a.L.cell_off);
    A.cells = reinterpret_cast<hsdev::AlleleCell*>(d_cells); A.cells_cap = cells_cap; A.n_calls = (int32_t*)(work + a.L.n_calls); A.n_snps = S;
    A.wide_count = (int32_t*)(work + a.wide_count); A.wide_list = (int32_t*)(work + a.wide_list);
    HS_HIP(hipMemsetAsync(A.wide_count, 0, 4, st));
    hipLaunchKernelGGL(hsdev::k_allele_cells, dim3((unsigned)S), dim3(64), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_allele_cells_wide, dim3(HS_ALLELE_WIDE_BLOCKS), dim3(256), 0, st, A, (uint32_t*)(work + a.slabs));
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// The recruit table behind the cells (hs_capi_recruit.inc): asked for with a RecruitReq, it shares the work buffer, the stream and both host waits
// (declared here, defined there: this file's stage-level route queues them between its own launches)
struct RecruitWork { AlleleWork a; hs_recruit_layout L; int64_t ctr_n, tile_sum; int n_tiles; };      // the parts of d_work behind the allele plan's (hs_recruit_layout)
struct RecruitReq { hs_recruit_params params; hs_recruit_table* table = nullptr; };
static RecruitWork recruit_work(int32_t S, int32_t W, int64_t n_labels);
static int recruit_plan_launch(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params, hipStream_t st);
static int recruit_rows_launch(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params, const hs_allele_cell* d_cells, int64_t cells_cap,
                               uint32_t* d_counters, int64_t counters_cap, hs_recruit_row* d_rows, int64_t rows_cap, hipStream_t st);
struct AlleleHostIn;
static int alleles_on_device(const AlleleHostIn& h, const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const int32_t* d_labels,
                             KernelClock& kc, hipStream_t st, hs_allele_table** out, RecruitReq* rq = nullptr);

// Host copies of what the call describes (the table is assembled from them) next to the device arrays
struct AlleleHostIn {
    std::vector<int32_t> win_contig, win_start, win_end, snp_contig, snp_pos;
    std::vector<uint8_t> snp_ref, snp_alt;
    std::vector<int64_t> win_off, label_off;
    int32_t contig_base = 0;
    int64_t n_entries = 0;
    int64_t groups_bound = 0;      // no more groups than this over all windows (labels >= 0 of the call: every group has a read)
};

// plan -> (one wait: the number of cells) -> cells -> (one wait) -> table. The columns and the dense labels are on the device already;
// the small per-SNP / per-window arrays of `h` are uploaded here. Launches are accounted under HS_K_OTHER.
static int alleles_on_device(const AlleleHostIn& h, const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const int32_t* d_labels,
                             KernelClock& kc, hipStream_t st, hs_allele_table** out, RecruitReq* rq) {
    const int64_t S64 = (int64_t)h.snp_pos.size(), W64 = (int64_t)h.win_start.size();
    if (S64 > 0x7fffffff || W64 > 0x7fffffff) { set_error("allele table: more than 2^31 SNPs or windows in one call"); return HS_EINVAL; }
    const int32_t S = (int32_t)S64, W = (int32_t)W64;
    const int32_t C = (int32_t)h.win_off.size() - 1;
    const int64_t n_labels = h.label_off.empty() ? 0 : h.label_off.back();
    if (rq && n_labels > 0x7fffffff - HS_SCAN_TILE) { set_error("recruit table: more than 2^31 labels in one call"); return HS_EINVAL; }
    const RecruitWork rw = rq ? recruit_work(S, W, n_labels) : RecruitWork();      // (its allele part is allele_work's: the recruit parts lie behind it)
    const AlleleWork a = rq ? rw.a : allele_work(S, W, n_labels);
    const size_t work_bytes = (size_t)(rq ? rw.L.total_bytes : a.L.total_bytes);
    DBuf d_work, d_sr, d_sa, d_sp, d_sc, d_wo, d_ws, d_we, d_lo, d_cells, d_counters, d_rows;
    UploadPack pk;
    pk.add(h.snp_ref, d_sr); pk.add(h.snp_alt, d_sa); pk.add(h.snp_pos, d_sp); pk.add(h.snp_contig, d_sc);
    pk.add(h.win_off, d_wo); pk.add(h.win_start, d_ws); pk.add(h.win_end, d_we); pk.add(h.label_off, d_lo);
    if (int rc = pk.commit(st)) return rc;
    if (int rc = d_work.alloc(work_bytes)) return rc;
    AlleleDevIn in{d_col_off, d_col_idx, d_col_code, d_sr.as<uint8_t>(), d_sa.as<uint8_t>(), d_sp.as<int32_t>(), d_sc.as<int32_t>(), S,
                   d_wo.as<int64_t>(), d_ws.as<int32_t>(), d_we.as<int32_t>(), C, W, d_lo.as<int64_t>(), d_labels, n_labels};
    char* work = (char*)d_work.p;
    EventPair ev_plan, ev, ev_rplan, ev_rrows;      // (the table's own kernel time: the plan's launches and the cells', not the wait between them)
    if (int rc = ev_plan.init()) return rc;
    if (int rc = ev.init()) return rc;
    if (rq) { if (int rc = ev_rplan.init()) return rc; if (int rc = ev_rrows.init()) return rc; }
    HS_HIP(ev_rec(ev_plan.a, st));
    if (int rc = kc.begin(HS_K_OTHER, st)) return rc;
    if (int rc = allele_plan_launch(in, work, a, st)) return rc;
    if (int rc = kc.end(4 * n_labels + 12 * (int64_t)S, st)) return rc;
    HS_HIP(ev_rec(ev_plan.b, st));
    if (rq) {      // the rows' flags and the two scans over them: queued with the plan, counted in the plan's wait
        HS_HIP(ev_rec(ev_rplan.a, st));
        if (int rc = kc.begin(HS_K_OTHER, st)) return rc;
        if (int rc = recruit_plan_launch(in, work, rw, rq->params, st)) return rc;
        if (int rc = kc.end(4 * h.n_entries + 40 * n_labels, st)) return rc;
        HS_HIP(ev_rec(ev_rplan.b, st));
    }
    // the plan comes to the host in one shipment (the table is assembled from it); its last word says how many cells to make room for
    const size_t plan_bytes = (size_t)a.L.n_calls;      // snp_win .. grp_off lie in front of n_calls; the packed group lists follow them on the host
    const int64_t groups_cap = std::min<int64_t>(std::max<int64_t>(h.groups_bound, 0), n_labels);      // (every group has a read)
    HBuf h_plan;
    const size_t totals_at = (plan_bytes + (size_t)groups_cap * 4 + 255) & ~(size_t)255;      // recruit: rows and counter words, behind the group lists
    if (int rc = h_plan.alloc(totals_at + 256)) return rc;
    {
        Shipment sh;
        sh.add(h_plan.p, work, plan_bytes);
        if (rq) {      // (a shipment moves 16-byte pieces: the piece each total lies in)
            sh.add((char*)h_plan.p + totals_at, work + rw.L.row_idx + ((n_labels * 8) & ~(int64_t)15), 16);
            sh.add((char*)h_plan.p + totals_at + 16, work + rw.L.ctr_off + ((n_labels * 8) & ~(int64_t)15), 16);
        }
        if (W && S) sh.add_counted((char*)h_plan.p + plan_bytes, work + a.L.grp_pack, (const long long*)(work + a.L.grp_off) + W, 4, groups_cap);
        if (int rc = sh.launch(st, 64)) return rc;
    }
    if (int rc = stream_wait(st)) return rc;
    const char* hp = (const char*)h_plan.p;
    const int64_t* cell_off = (const int64_t*)(hp + a.L.cell_off);
    const int64_t* grp_off = (const int64_t*)(hp + a.L.grp_off);
    const int64_t n_cells = cell_off[S];
    if (n_cells < 0 || grp_off[W] < 0 || grp_off[W] > groups_cap) { set_error("allele table: the device's group lists do not fit the labels of the call"); return HS_EHIP; }
    if (int rc = d_cells.alloc((size_t)std::max<int64_t>(n_cells, 1) * sizeof(hs_allele_cell) + 16)) return rc;
    const size_t in_piece = (size_t)((n_labels * 8) & 15);
    const int64_t n_rows = rq ? *(const int64_t*)(hp + totals_at + in_piece) : 0, n_ctr = rq ? *(const int64_t*)(hp + totals_at + 16 + in_piece) : 0;
    if (rq) {
        if (n_rows < 0 || n_rows > n_labels || n_ctr < n_rows) { set_error("recruit table: the device's row counts do not fit the labels of the call"); return HS_EHIP; }
        if (int rc = d_counters.alloc((size_t)std::max<int64_t>(n_ctr, 1) * 4)) return rc;
        if (int rc = d_rows.alloc((size_t)std::max<int64_t>(n_rows, 1) * sizeof(hs_recruit_row))) return rc;
    }
    HS_HIP(ev_rec(ev.a, st));
    if (int rc = kc.begin(HS_K_OTHER, st)) return rc;
    if (int rc = allele_cells_launch(in, work, a, d_cells.as<hs_allele_cell>(), n_cells, st)) return rc;
    if (int rc = kc.end(5 * h.n_entries + (int64_t)sizeof(hs_allele_cell) * n_cells, st)) return rc;
    HS_HIP(ev_rec(ev.b, st));
    HBuf h_rows;
    const size_t rows_bytes = (size_t)n_rows * sizeof(hs_recruit_row), wro_at = (rows_bytes + 255) & ~(size_t)255, status_at = wro_at + ((((size_t)W + 1) * 8 + 255) & ~(size_t)255);
    if (rq) {      // counters and rows behind the cells; they come down in the cells' shipment
        HS_HIP(ev_rec(ev_rrows.a, st));
        if (int rc = kc.begin(HS_K_OTHER, st)) return rc;
        if (int rc = recruit_rows_launch(in, work, rw, rq->params, d_cells.as<hs_allele_cell>(), n_cells, d_counters.as<uint32_t>(), n_ctr, d_rows.as<hs_recruit_row>(), n_rows, st)) return rc;
        if (int rc = kc.end(5 * h.n_entries + 12 * n_ctr + 40 * n_rows + 12 * n_labels, st)) return rc;
        HS_HIP(ev_rec(ev_rrows.b, st));
        if (int rc = h_rows.alloc(status_at + 256)) return rc;
    }
    const size_t cells_bytes = (size_t)n_cells * sizeof(hs_allele_cell), calls_bytes = (size_t)S * 4;
    HBuf h_cells;
    const size_t calls_at = (cells_bytes + 255) & ~(size_t)255;
    if (int rc = h_cells.alloc(calls_at + ((calls_bytes + 255) & ~(size_t)255) + 256)) return rc;
    {
        Shipment sh;
        sh.add(h_cells.p, d_cells.p, cells_bytes); sh.add((char*)h_cells.p + calls_at, work + a.L.n_calls, calls_bytes);
        sh.add((char*)h_cells.p + calls_at + ((calls_bytes + 255) & ~(size_t)255), work + a.wide_count, 4);
        if (rq) { sh.add(h_rows.p, d_rows.p, rows_bytes); sh.add((char*)h_rows.p + wro_at, work + rw.L.win_row_off, ((size_t)W + 1) * 8); sh.add((char*)h_rows.p + status_at, work + rw.L.status, 4); }
        if (int rc = sh.launch(st, 64)) return rc;
    }
    if (int rc = stream_wait(st)) return rc;
    kc.flush();
    hs::AlleleRaw raw;
    raw.n_windows = W; raw.n_snps = S;
    raw.win_contig = h.win_contig.data(); raw.win_start = h.win_start.data(); raw.win_end = h.win_end.data(); raw.grp_off = grp_off;
    raw.grp_n = (const int32_t*)(hp + a.L.grp_n); raw.grp_ids = (const int32_t*)(hp + plan_bytes);
    raw.win_snp_first = (const int32_t*)(hp + a.L.win_snp_first); raw.win_snp_last = (const int32_t*)(hp + a.L.win_snp_last);
    raw.snp_contig = h.snp_contig.data(); raw.snp_pos = h.snp_pos.data(); raw.snp_ref = h.snp_ref.data(); raw.snp_alt = h.snp_alt.data();
    raw.snp_win = (const int32_t*)(hp + a.L.snp_win); raw.cell_off = cell_off;
    raw.cells = (const hs_allele_cell*)h_cells.p; raw.n_calls = (const int32_t*)((const char*)h_cells.p + calls_at);
    raw.contig_base = h.contig_base;
    std::string err;
    hs_allele_table* t = hs::alleles_assemble(raw, err);
    if (!t) { set_error(err); return HS_EINVAL; }
    float ms = 0, ms_plan = 0;
    if (int rc = ev.ms(&ms)) { hs::alleles_free(t); return rc; }
    if (int rc = ev_plan.ms(&ms_plan)) { hs::alleles_free(t); return rc; }
    t->t_kernel_ms = (double)ms + ms_plan; t->n_entries = h.n_entries;
    t->n_wide_columns = S && W ? *(const int32_t*)((const char*)h_cells.p + calls_at + ((calls_bytes + 255) & ~(size_t)255)) : 0;
    if (rq) {
        hs::RecruitRaw rr;
        rr.n_windows = W; rr.win_contig = h.win_contig.data(); rr.win_start = h.win_start.data(); rr.win_end = h.win_end.data();
        rr.win_snp_first = raw.win_snp_first; rr.win_snp_last = raw.win_snp_last;
        rr.win_row_off = (const int64_t*)((const char*)h_rows.p + wro_at); rr.rows = (const hs_recruit_row*)h_rows.p;
        rr.contig_base = h.contig_base; rr.params = rq->params;
        hs_recruit_table* rt = nullptr;
        if (*(const int32_t*)((const char*)h_rows.p + status_at) != 0) err = "recruit table: the rows or counters did not fit their arrays";
        else rt = hs::recruit_assemble(rr, err);
        float ms_a = 0, ms_b = 0;
        if (rt && (ev_rplan.ms(&ms_a) || ev_rrows.ms(&ms_b))) { hs::recruit_free(rt); hs::alleles_free(t); return HS_EHIP; }
        if (!rt) { hs::alleles_free(t); set_error(err); return HS_EINVAL; }
        rt->t_kernel_ms = (double)ms_a + ms_b; rt->n_counter_words = n_ctr; rt->n_entries = h.n_entries;
        rq->table = rt;
    }
    *out = t;
    return HS_OK;
}

// dense labels on the device from the per-window lists a contig group leaves (SrSparseLabels)
static int allele_dense_labels(const hs::SrSparseLabels& sp, const std::vector<int64_t>& label_off, DBuf& d_labels, UploadPack& pk, DBuf& d_ro, DBuf& d_ids,
                               DBuf& d_lab, DBuf& d_lo, hipStream_t st) {
    const int64_t W = (int64_t)label_off.size() - 1, n = label_off.back();
    if (int rc = d_labels.alloc((size_t)std::max<int64_t>(n, 1) * 4)) return rc;
    if (W <= 0 || n <= 0) return HS_OK;
    pk.add(sp.off, d_ro); pk.add(sp.ids, d_ids); pk.add(sp.labels, d_lab); pk.add(label_off, d_lo);
    if (int rc = pk.commit(st)) return rc;
    hipLaunchKernelGGL(hsdev::k_allele_fill_absent, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (n + 255) / 256))), dim3(256), 0, st, d_labels.as<int32_t>(), (long long)n);
    hipLaunchKernelGGL(hsdev::k_allele_scatter_labels, dim3((unsigned)W), dim3(256), 0, st, d_ro.as<int64_t>(), d_ids.as<int32_t>(), d_lab.as<int32_t>(),
                       d_lo.as<int64_t>(), (int)W, d_labels.as<int32_t>());
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// The share of one contig group of a pipeline, at the end of its chain: the SNP columns are the ones stage 4 read on the device (`ops`: taken
// over from stage 3 where it packed them, or uploaded by stage 4 -- HS_COLUMNS_VIA_HOST, HS_PIPELINE_KEEP_COLUMNS, a group that lost SNPs to
// rarest_strain_abundance), the labels go up as the per-window lists the group leaves and are spread on the device. `r` / `sp`: the group's
// stage-4 result; `cv`: its stage-3 result (contigs [c0, c0 + r->n_contigs) of the batch).
static int pipeline_group_alleles(const hs_sr_result* r, const hs::SrSparseLabels& sp, const hs_cv_result* cv, float rsa, int c0, HipSrOps& ops, hs_allele_table** out,
                                  RecruitReq* rq = nullptr) {
    const int C = r->n_contigs;
    AlleleHostIn h;
    h.contig_base = c0;
    const int64_t W = r->win_off[C];
    h.win_off.assign(r->win_off, r->win_off + C + 1);
    h.win_start.assign(r->win_start, r->win_start + W); h.win_end.assign(r->win_end, r->win_end + W);
    h.label_off.assign(r->label_off, r->label_off + W + 1);
    h.win_contig.resize((size_t)W);
    for (int c = 0; c < C; ++c) for (int64_t w = r->win_off[c]; w < r->win_off[c + 1]; ++w) h.win_contig[(size_t)w] = c;
    for (int c = 0; c < C; ++c)
        for (int64_t s = cv->snp_off[c]; s < cv->snp_off[c + 1]; ++s) {
            if (!hs::snp_kept_by_abundance(cv->snp_n_ref[s], cv->snp_n_alt[s], rsa)) continue;
            h.snp_contig.push_back(c); h.snp_pos.push_back(cv->snp_pos[s]); h.snp_ref.push_back(cv->snp_ref[s]); h.snp_alt.push_back(cv->snp_alt[s]);
            h.n_entries += cv->col_off[s + 1] - cv->col_off[s];
        }
    h.groups_bound = (int64_t)sp.ids.size();
    if ((int64_t)sp.off.size() != W + 1) { set_error("allele table: the group's labels do not describe its windows"); return HS_EINVAL; }
    if (!h.snp_pos.empty() && W > 0 && (!ops.d_col_off.p || !ops.d_col_idx.p || !ops.d_col_code.p)) { set_error("allele table: stage 4 left no SNP columns on the device"); return HS_EINVAL; }
    if (h.snp_pos.empty() || W == 0) {      // nothing to cross: an empty table, no launch
        hs::AlleleRaw raw;
        std::string err;
        const int64_t zero = 0;
        raw.cell_off = &zero;
        *out = hs::alleles_assemble(raw, err);
        if (!*out) { set_error(err); return HS_EINVAL; }
        if (rq) {      // (no rows either; the table still says how many windows the group has)
            const std::vector<int32_t> none((size_t)W + 1, 0);
            const std::vector<int64_t> row_off((size_t)W + 1, 0);
            hs::RecruitRaw rr;
            rr.n_windows = W; rr.win_contig = h.win_contig.data(); rr.win_start = h.win_start.data(); rr.win_end = h.win_end.data();
            rr.win_snp_first = none.data(); rr.win_snp_last = none.data(); rr.win_row_off = row_off.data(); rr.contig_base = c0; rr.params = rq->params;
            rq->table = hs::recruit_assemble(rr, err);
            if (!rq->table) { set_error(err); return HS_EINVAL; }
        }
        return HS_OK;
    }
    DBuf d_labels, d_ro, d_ids, d_lab, d_lo;
    UploadPack pk;
    if (int rc = allele_dense_labels(sp, h.label_off, d_labels, pk, d_ro, d_ids, d_lab, d_lo, ops.stream)) return rc;
    return alleles_on_device(h, ops.d_col_off.as<int64_t>(), ops.d_col_idx.as<int32_t>(), ops.d_col_code.as<uint8_t>(), d_labels.as<int32_t>(), ops.kc, ops.stream, out, rq);
}

}  // namespace

extern "C" {

int32_t hs_alleles_lds_capacity(void) { return HS_ALLELE_LDS_KEYS; }

int hs_group_alleles_layout(int32_t n_snps, int32_t n_windows, int64_t n_labels, hs_allele_layout* out) {
    if (!out || n_snps < 0 || n_windows < 0 || n_labels < 0) { set_error("hs_group_alleles_layout: bad arguments"); return HS_EINVAL; }
    *out = allele_work(n_snps, n_windows, n_labels).L;
    return HS_OK;
}

int hs_group_alleles(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const uint8_t* d_snp_ref, const uint8_t* d_snp_alt,
                     const int32_t* d_snp_pos, const int32_t* d_snp_contig, int32_t n_snps, const int64_t* d_win_off, const int32_t* d_win_start,
                     const int32_t* d_win_end, int32_t n_contigs, int32_t n_windows, const int64_t* d_label_off, const int32_t* d_labels, int64_t n_labels,
                     void* d_work, hs_allele_cell* d_cells, int64_t cells_cap, void* stream) {
    if (int rc = require_device()) return rc;
    if (n_snps < 0 || n_windows < 0 || n_contigs < 0 || n_labels < 0 || !d_work || (d_cells && cells_cap < 0)) { set_error("hs_group_alleles: bad arguments"); return HS_EINVAL; }
    const AlleleWork a = allele_work(n_snps, n_windows, n_labels);
    const AlleleDevIn in{d_col_off, d_col_idx, d_col_code, d_snp_ref, d_snp_alt, d_snp_pos, d_snp_contig, n_snps, d_win_off, d_win_start, d_win_end,
                         n_contigs, n_windows, d_label_off, d_labels, n_labels};
    // (asynchronous: nothing here waits for the launches, so nothing times them either -- the stage-level callers account them under HS_K_OTHER)
    hipStream_t st = (hipStream_t)stream;
    return d_cells ? allele_cells_launch(in, (char*)d_work, a, d_cells, cells_cap, st) : allele_plan_launch(in, (char*)d_work, a, st);
}

// (hs_recruit_reads of hs_capi_recruit.inc is the same call with a RecruitReq)
static int haplotype_tables(const hs_sr_contig* contigs, int32_t n_contigs, const hs_sr_result* sr, hs_allele_table** table, RecruitReq* rq) {
    if (int rc = require_device()) return rc;
    if (!contigs || !sr || !table || n_contigs < 0 || sr->n_contigs != n_contigs) { set_error("hs_haplotype_alleles: the result does not describe these contigs"); return HS_EINVAL; }
    if (!sr->labels && sr->win_off[n_contigs] > 0 && sr->label_off[sr->win_off[n_contigs]] > 0) { set_error("hs_haplotype_alleles: the result has no dense labels"); return HS_EINVAL; }
    AlleleHostIn h;
    const int64_t W = sr->win_off[n_contigs];
    h.win_off.assign(sr->win_off, sr->win_off + n_contigs + 1);
    h.win_start.assign(sr->win_start, sr->win_start + W); h.win_end.assign(sr->win_end, sr->win_end + W);
    h.label_off.assign(sr->label_off, sr->label_off + W + 1);
    h.win_contig.resize((size_t)W);
    std::vector<int64_t> col_off(1, 0);
    for (int c = 0; c < n_contigs; ++c) {
        const hs_sr_contig& k = contigs[c];
        if (sr->win_off[c + 1] < sr->win_off[c] || k.n_snps < 0 || k.n_reads < 0) { set_error("hs_haplotype_alleles: bad contig"); return HS_EINVAL; }
        for (int64_t w = sr->win_off[c]; w < sr->win_off[c + 1]; ++w) {
            h.win_contig[(size_t)w] = c;
            if (sr->label_off[w + 1] - sr->label_off[w] != k.n_reads) { set_error("hs_haplotype_alleles: a window's labels are not one per read of its contig"); return HS_EINVAL; }
            if (w > sr->win_off[c] && (sr->win_start[w] <= sr->win_end[w - 1] || sr->win_end[w] < sr->win_start[w])) { set_error("hs_haplotype_alleles: the windows of a contig must ascend without overlap"); return HS_EINVAL; }
        }
        for (int s = 0; s < k.n_snps; ++s) {
            const int64_t d = k.col_off[s + 1] - k.col_off[s];
            if (d < 0 || d > 65535) { set_error("hs_haplotype_alleles: a column with more than 65535 entries"); return HS_EINVAL; }
            if (s > 0 && k.snp_pos[s] < k.snp_pos[s - 1]) { set_error("hs_haplotype_alleles: SNP positions must ascend on every contig"); return HS_EINVAL; }
            col_off.push_back(col_off.back() + d);
            h.snp_contig.push_back(c); h.snp_pos.push_back(k.snp_pos[s]); h.snp_ref.push_back(k.snp_ref[s]); h.snp_alt.push_back(k.snp_alt[s]);
        }
    }
    h.n_entries = col_off.back();
    std::vector<int32_t> col_idx((size_t)h.n_entries); std::vector<uint8_t> col_code((size_t)h.n_entries);
    {
        size_t s = 0;
        for (int c = 0; c < n_contigs; ++c) {
            const hs_sr_contig& k = contigs[c];
            if (k.n_snps == 0) continue;
            const int64_t n = k.col_off[k.n_snps] - k.col_off[0];
            if (n) { std::memcpy(col_idx.data() + col_off[s], k.col_idx + k.col_off[0], (size_t)n * 4); std::memcpy(col_code.data() + col_off[s], k.col_code + k.col_off[0], (size_t)n); }
            s += (size_t)k.n_snps;
        }
    }
    hipStream_t st = nullptr;
    DBuf d_co, d_ci, d_cc, d_labels;
    if (int rc = d_co.upload(col_off)) return rc;
    if (int rc = d_ci.upload(col_idx)) return rc;
    if (int rc = d_cc.upload(col_code)) return rc;
    {
        const int64_t n = h.label_off.back();
        if (int rc = d_labels.alloc((size_t)std::max<int64_t>(n, 1) * 4)) return rc;
        for (int64_t i = 0; i < n; ++i) h.groups_bound += sr->labels[i] >= 0;
        if (n > 0) {      // (staged through pinned memory in pieces: the labels of a large job are tens of megabytes)
            HBuf hb;
            const int64_t piece = (int64_t)16 << 20;
            if (int rc = hb.alloc((size_t)std::min<int64_t>(n, piece) * 4)) return rc;
            for (int64_t o = 0; o < n; o += piece) {
                const int64_t m = std::min<int64_t>(piece, n - o);
                std::memcpy(hb.p, sr->labels + o, (size_t)m * 4);
                HS_HIP(hipMemcpy((int32_t*)d_labels.p + o, hb.p, (size_t)m * 4, hipMemcpyHostToDevice));
            }
        }
    }
    KernelClock kc;
    return alleles_on_device(h, d_co.as<int64_t>(), d_ci.as<int32_t>(), d_cc.as<uint8_t>(), d_labels.as<int32_t>(), kc, st, table, rq);
}

int hs_haplotype_alleles(const hs_sr_contig* contigs, int32_t n_contigs, const hs_sr_result* sr, hs_allele_table** table) {
    return haplotype_tables(contigs, n_contigs, sr, table, nullptr);
}

}  // extern "C"
