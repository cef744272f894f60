// hs_capi_alleles.inc -- part of hs_capi.hip: the allele table (include/hairsplitter_hip.h: hs_group_alleles, hs_haplotype_alleles, and the
// share of a contig group of a pipeline). Kernels in hs_kernels_alleles.hip, the host side of the table in hs_alleles_host.cpp.
static_assert(sizeof(hs_allele_cell) == sizeof(hsdev::AlleleCell) && sizeof(hs_allele_cell) == 12, "hs_allele_cell layout");

namespace {

// the two tables of one call (or of one contig group of a pipeline), until somebody takes them over: what is still here when the holder goes is freed
struct TableFree { void operator()(hs_allele_table* t) const { hs::alleles_free(t); } void operator()(hs_recruit_table* t) const { hs::recruit_free(t); } };
struct TablePair { std::unique_ptr<hs_allele_table, TableFree> alleles; std::unique_ptr<hs_recruit_table, TableFree> recruit; };

// the parts of a work buffer, one after the other: 256-byte aligned, 4 bytes at least
struct WorkParts {
    int64_t o = 0;
    int64_t take(int64_t bytes) { const int64_t at = o; o = (o + std::max<int64_t>(bytes, 4) + 255) & ~(int64_t)255; return at; }
};
// the parts of d_work (hs_allele_layout). The small arrays lie in front (they go to the host in one shipment), then the
// group lists per window (room for one group per read) and one after the other; `internal`: has_snp [W], n_cells [S], the scans' tile sums
// and offsets, the wide route's counter and list [S], then its slabs
struct AlleleWork {
    hs_allele_layout L;
    int64_t has_snp, n_cells, tile_sum, wide_count, wide_list, slabs;
};
static AlleleWork allele_work(int32_t S, int32_t W, int64_t n_labels) {
    AlleleWork a;
    WorkParts p;
    a.L.snp_win = p.take((int64_t)S * 4); a.L.grp_n = p.take((int64_t)W * 4);
    a.L.win_snp_first = p.take((int64_t)W * 4); a.L.win_snp_last = p.take((int64_t)W * 4);      // (the two lie back to back: one clearing)
    a.L.cell_off = p.take(((int64_t)S + 1) * 8); a.L.grp_off = p.take(((int64_t)W + 1) * 8); a.L.n_calls = p.take((int64_t)S * 4);
    a.L.grp_ids = p.take(n_labels * 4); a.L.grp_pack = p.take(n_labels * 4);
    a.L.internal = p.o;
    a.has_snp = p.take((int64_t)W * 4); a.n_cells = p.take((int64_t)S * 4); a.tile_sum = p.take((int64_t)std::max(scan_tiles(std::max(S, W)), 1) * 16);
    a.wide_count = p.take(4); a.wide_list = p.take((int64_t)S * 4);
    a.slabs = p.take((int64_t)HS_ALLELE_WIDE_BLOCKS * HS_ALLELE_WIDE_KEYS * 4);
    a.L.total_bytes = p.o;
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
    if (int rc = exclusive_scan_launch(n_cells, S, cell_off, tile_sum, st)) return rc;
    if (int rc = exclusive_scan_launch(grp_n, W, grp_off, tile_sum, st)) return rc;      // (it takes the tile scratch over: the stream orders it behind the first)
    hipLaunchKernelGGL(hsdev::k_allele_pack_groups, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, grp_n, grp_off, in.d_label_off, grp_ids, W, grp_pack);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// what the column kernels of both tables read, from the call and the plan in `work`
static void column_args(const AlleleDevIn& in, char* work, const AlleleWork& a, int64_t cells_cap, hsdev::ColumnArgs& A) {
    A.col_off = in.d_col_off; A.col_idx = in.d_col_idx; A.col_code = in.d_col_code; A.n_snps = in.n_snps;
    A.snp_win = (const int32_t*)(work + a.L.snp_win); A.label_off = in.d_label_off; A.labels = in.d_labels; A.n_labels = in.n_labels; A.n_windows = in.n_windows;
    A.grp_n = (const int32_t*)(work + a.L.grp_n); A.grp_ids = (const int32_t*)(work + a.L.grp_ids); A.cell_off = (const int64_t*)(work + a.L.cell_off);
    A.cells_cap = cells_cap;
}

// the cells of the plan in `work`
static int allele_cells_launch(const AlleleDevIn& in, char* work, const AlleleWork& a, hs_allele_cell* d_cells, int64_t cells_cap, hipStream_t st) {
    const int S = in.n_snps;
    if (S == 0) return HS_OK;
    if (in.n_windows == 0) { HS_HIP(hipMemsetAsync(work + a.L.n_calls, 0, (size_t)S * 4, st)); return HS_OK; }
    hsdev::AlleleArgs A;
    column_args(in, work, a, cells_cap, A);
    A.snp_ref = in.d_snp_ref; A.snp_alt = in.d_snp_alt; A.cells = reinterpret_cast<hsdev::AlleleCell*>(d_cells); A.n_calls = (int32_t*)(work + a.L.n_calls);
    A.wide_count = (int32_t*)(work + a.wide_count); A.wide_list = (int32_t*)(work + a.wide_list);
    HS_HIP(hipMemsetAsync(A.wide_count, 0, 4, st));
    hipLaunchKernelGGL(hsdev::k_allele_cells, dim3((unsigned)S), dim3(64), 0, st, A);
    hipLaunchKernelGGL(hsdev::k_allele_cells_wide, dim3(HS_ALLELE_WIDE_BLOCKS), dim3(256), 0, st, A, (uint32_t*)(work + a.slabs));
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// The recruit table behind the cells (hs_capi_recruit.inc): asked for with its thresholds, it shares the work buffer, the stream and both host waits
// (declared here, defined there: this file's stage-level route queues them between its own launches)
struct RecruitWork { AlleleWork a; hs_recruit_layout L; int64_t ctr_n, tile_sum; };      // the parts of d_work behind the allele plan's (hs_recruit_layout)
static RecruitWork recruit_work(int32_t S, int32_t W, int64_t n_labels);
static int recruit_plan_launch(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params, hipStream_t st);
static int recruit_rows_launch(const AlleleDevIn& in, char* work, const RecruitWork& rw, const hs_recruit_params& params, const hs_allele_cell* d_cells, int64_t cells_cap,
                               uint32_t* d_counters, int64_t counters_cap, hs_recruit_row* d_rows, int64_t rows_cap, hipStream_t st);

// Host copies of what the call describes (the table is assembled from them) next to the device arrays
struct AlleleHostIn {
    std::vector<int32_t> win_contig, win_start, win_end, snp_contig, snp_pos;
    std::vector<uint8_t> snp_ref, snp_alt;
    std::vector<int64_t> win_off, label_off;
    int32_t contig_base = 0;
    int64_t n_entries = 0;
    int64_t groups_bound = 0;      // no more groups than this over all windows (labels >= 0 of the call: every group has a read)
    void windows_of(const hs_sr_result* r) {      // (win_contig: the caller's, it walks the contigs anyway)
        const int64_t W = r->win_off[r->n_contigs];
        win_off.assign(r->win_off, r->win_off + r->n_contigs + 1);
        win_start.assign(r->win_start, r->win_start + W); win_end.assign(r->win_end, r->win_end + W);
        label_off.assign(r->label_off, r->label_off + W + 1);
        win_contig.resize((size_t)W);
    }
};

// Where the two shipments of a stage-level call land in pinned host memory: byte offsets, 256-byte aligned. The first goes to one block:
// the front of the work buffer as it lies on the device (snp_win .. grp_off, all in front of n_calls: the fields of hs_allele_layout hold
// there too), the packed group lists, the 16-byte pieces of the recruit table's two totals. The second is sized by those totals and
// goes to two blocks: cells, n_calls and the wide route's counter; rows, win_row_off and status.
struct TableLanding {
    int64_t groups_cap;      // (every group has a read)
    size_t plan_bytes, grp_pack, n_rows_piece, n_ctr_piece, plan_size;
    size_t cells_bytes, n_calls, calls_bytes, wide_count, cells_size;
    size_t rows_bytes, win_row_off, win_row_off_bytes, status, rows_size;
};
static TableLanding table_landing(const AlleleWork& a, int32_t S, int32_t W, int64_t groups_cap, int64_t n_cells = 0, int64_t n_rows = 0) {
    const auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
    TableLanding t;
    t.groups_cap = groups_cap;
    t.plan_bytes = (size_t)a.L.n_calls; t.grp_pack = t.plan_bytes;
    t.n_rows_piece = up(t.grp_pack + (size_t)groups_cap * 4); t.n_ctr_piece = t.n_rows_piece + 16; t.plan_size = t.n_rows_piece + 256;
    t.cells_bytes = (size_t)n_cells * sizeof(hs_allele_cell); t.calls_bytes = (size_t)S * 4;
    t.n_calls = up(t.cells_bytes); t.wide_count = t.n_calls + up(t.calls_bytes); t.cells_size = t.wide_count + 256;
    t.rows_bytes = (size_t)n_rows * sizeof(hs_recruit_row); t.win_row_off_bytes = ((size_t)W + 1) * 8;
    t.win_row_off = up(t.rows_bytes); t.status = t.win_row_off + up(t.win_row_off_bytes); t.rows_size = t.status + 256;
    return t;
}

// One stage-level call between its parts: plan -> (one wait: the totals) -> cells, and rows behind them -> (one wait) -> the tables. The
// columns and the dense labels are on the device already; the small per-SNP / per-window arrays of `h` are uploaded here. With `recruit`
// (its thresholds; nullptr: the allele table alone) the recruit table's launches are queued behind the allele table's, in the same two
// shipments. Launches are accounted under HS_K_OTHER.
struct TableCall {
    const AlleleHostIn& h; const hs_recruit_params* recruit; KernelClock& kc; hipStream_t st;
    int32_t S = 0, W = 0;
    int64_t n_labels = 0, n_cells = 0, n_rows = 0, n_ctr = 0;
    RecruitWork rw;      // (its allele part is allele_work's: the recruit parts lie behind it)
    TableLanding at;
    AlleleDevIn in;
    DBuf d_work, d_sr, d_sa, d_sp, d_sc, d_wo, d_ws, d_we, d_lo, d_cells, d_counters, d_rows;
    UploadPack pk;
    HBuf h_plan, h_cells, h_rows;
    EventPair ev_plan, ev_cells, ev_rplan, ev_rrows;      // (the tables' own kernel time: the plans' launches and the cells' and rows', not the wait between them)
    const int64_t* h_n_rows = nullptr; const int64_t* h_n_ctr = nullptr;      // the two totals where the first shipment leaves them

    char* work() const { return (char*)d_work.p; }

    // uploads, the plan(s), and their shipment: the plan comes to the host in one piece (the table is assembled from it) with the totals that size the rest
    int queue_plan(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const int32_t* d_labels) {
        const int64_t S64 = (int64_t)h.snp_pos.size(), W64 = (int64_t)h.win_start.size();
        if (S64 > 0x7fffffff || W64 > 0x7fffffff) { set_error("allele table: more than 2^31 SNPs or windows in one call"); return HS_EINVAL; }
        S = (int32_t)S64; W = (int32_t)W64;
        n_labels = h.label_off.empty() ? 0 : h.label_off.back();
        if (recruit && n_labels > 0x7fffffff - HS_SCAN_TILE) { set_error("recruit table: more than 2^31 labels in one call"); return HS_EINVAL; }
        rw = recruit_work(S, W, n_labels);
        at = table_landing(rw.a, S, W, std::min<int64_t>(std::max<int64_t>(h.groups_bound, 0), n_labels));
        pk.add(h.snp_ref, d_sr); pk.add(h.snp_alt, d_sa); pk.add(h.snp_pos, d_sp); pk.add(h.snp_contig, d_sc);
        pk.add(h.win_off, d_wo); pk.add(h.win_start, d_ws); pk.add(h.win_end, d_we); pk.add(h.label_off, d_lo);
        if (int rc = pk.commit(st)) return rc;
        if (int rc = d_work.alloc((size_t)(recruit ? rw.L.total_bytes : rw.a.L.total_bytes))) return rc;
        in = AlleleDevIn{d_col_off, d_col_idx, d_col_code, d_sr.as<uint8_t>(), d_sa.as<uint8_t>(), d_sp.as<int32_t>(), d_sc.as<int32_t>(), S,
                         d_wo.as<int64_t>(), d_ws.as<int32_t>(), d_we.as<int32_t>(), (int32_t)h.win_off.size() - 1, W, d_lo.as<int64_t>(), d_labels, n_labels};
        if (int rc = ev_plan.init()) return rc;
        if (int rc = ev_cells.init()) return rc;
        if (recruit) { if (int rc = ev_rplan.init()) return rc; if (int rc = ev_rrows.init()) return rc; }
        if (int rc = timed_launch(kc, ev_plan, st, 4 * n_labels + 12 * (int64_t)S, [&] { return allele_plan_launch(in, work(), rw.a, st); })) return rc;
        // (the rows' flags and the two scans over them: queued with the plan, counted in the plan's wait)
        if (recruit) { if (int rc = timed_launch(kc, ev_rplan, st, 4 * h.n_entries + 40 * n_labels, [&] { return recruit_plan_launch(in, work(), rw, *recruit, st); })) return rc; }
        if (int rc = h_plan.alloc(at.plan_size)) return rc;
        char* hp = (char*)h_plan.p;
        Shipment sh;
        sh.add(hp, work(), at.plan_bytes);
        if (recruit) {
            h_n_rows = sh.add_word(hp + at.n_rows_piece, (const int64_t*)(work() + rw.L.row_idx) + n_labels);
            h_n_ctr = sh.add_word(hp + at.n_ctr_piece, (const int64_t*)(work() + rw.L.ctr_off) + n_labels);
        }
        if (W && S) sh.add_counted(hp + at.grp_pack, work() + rw.a.L.grp_pack, (const long long*)(work() + rw.a.L.grp_off) + W, 4, at.groups_cap);
        return sh.launch(st, 64);
    }

    // behind the first wait: the totals, and room for what they count
    int size_buffers() {
        const char* hp = (const char*)h_plan.p;
        const int64_t n_groups = ((const int64_t*)(hp + rw.a.L.grp_off))[W];
        n_cells = ((const int64_t*)(hp + rw.a.L.cell_off))[S];
        if (n_cells < 0 || n_groups < 0 || n_groups > at.groups_cap) { set_error("allele table: the device's group lists do not fit the labels of the call"); return HS_EHIP; }
        if (int rc = d_cells.alloc((size_t)std::max<int64_t>(n_cells, 1) * sizeof(hs_allele_cell) + 16)) return rc;
        if (recruit) {
            n_rows = *h_n_rows; n_ctr = *h_n_ctr;
            if (n_rows < 0 || n_rows > n_labels || n_ctr < n_rows) { set_error("recruit table: the device's row counts do not fit the labels of the call"); return HS_EHIP; }
            if (int rc = d_counters.alloc((size_t)std::max<int64_t>(n_ctr, 1) * 4)) return rc;
            if (int rc = d_rows.alloc((size_t)std::max<int64_t>(n_rows, 1) * sizeof(hs_recruit_row))) return rc;
        }
        at = table_landing(rw.a, S, W, at.groups_cap, n_cells, n_rows);
        return HS_OK;
    }

    // the cells, counters and rows behind them, and their shipment
    int queue_cells() {
        hs_allele_cell* cells = d_cells.as<hs_allele_cell>();
        if (int rc = timed_launch(kc, ev_cells, st, 5 * h.n_entries + (int64_t)sizeof(hs_allele_cell) * n_cells, [&] { return allele_cells_launch(in, work(), rw.a, cells, n_cells, st); })) return rc;
        if (recruit) {
            if (int rc = timed_launch(kc, ev_rrows, st, 5 * h.n_entries + 12 * n_ctr + 40 * n_rows + 12 * n_labels, [&] {
                    return recruit_rows_launch(in, work(), rw, *recruit, cells, n_cells, d_counters.as<uint32_t>(), n_ctr, d_rows.as<hs_recruit_row>(), n_rows, st); })) return rc;
            if (int rc = h_rows.alloc(at.rows_size)) return rc;
        }
        if (int rc = h_cells.alloc(at.cells_size)) return rc;
        char* hc = (char*)h_cells.p; char* hr = (char*)h_rows.p;
        Shipment sh;
        sh.add(hc, d_cells.p, at.cells_bytes); sh.add(hc + at.n_calls, work() + rw.a.L.n_calls, at.calls_bytes); sh.add(hc + at.wide_count, work() + rw.a.wide_count, 4);
        if (recruit) { sh.add(hr, d_rows.p, at.rows_bytes); sh.add(hr + at.win_row_off, work() + rw.L.win_row_off, at.win_row_off_bytes); sh.add(hr + at.status, work() + rw.L.status, 4); }
        return sh.launch(st, 64);
    }

    // behind the second wait: the tables from what the two shipments left (an error leaves what exists to the holder)
    int assemble(TablePair& out) {
        const char* hp = (const char*)h_plan.p; const char* hc = (const char*)h_cells.p; const char* hr = (const char*)h_rows.p;
        hs::AlleleRaw raw;
        raw.n_windows = W; raw.n_snps = S;
        raw.win_contig = h.win_contig.data(); raw.win_start = h.win_start.data(); raw.win_end = h.win_end.data(); raw.grp_off = (const int64_t*)(hp + rw.a.L.grp_off);
        raw.grp_n = (const int32_t*)(hp + rw.a.L.grp_n); raw.grp_ids = (const int32_t*)(hp + at.grp_pack);
        raw.win_snp_first = (const int32_t*)(hp + rw.a.L.win_snp_first); raw.win_snp_last = (const int32_t*)(hp + rw.a.L.win_snp_last);
        raw.snp_contig = h.snp_contig.data(); raw.snp_pos = h.snp_pos.data(); raw.snp_ref = h.snp_ref.data(); raw.snp_alt = h.snp_alt.data();
        raw.snp_win = (const int32_t*)(hp + rw.a.L.snp_win); raw.cell_off = (const int64_t*)(hp + rw.a.L.cell_off);
        raw.cells = (const hs_allele_cell*)hc; raw.n_calls = (const int32_t*)(hc + at.n_calls);
        raw.contig_base = h.contig_base;
        std::string err;
        out.alleles.reset(hs::alleles_assemble(raw, err));
        if (!out.alleles) { set_error(err); return HS_EINVAL; }
        float ms = 0, ms_plan = 0;
        if (int rc = ev_cells.ms(&ms)) return rc;
        if (int rc = ev_plan.ms(&ms_plan)) return rc;
        out.alleles->t_kernel_ms = (double)ms + ms_plan; out.alleles->n_entries = h.n_entries;
        out.alleles->n_wide_columns = S && W ? *(const int32_t*)(hc + at.wide_count) : 0;
        if (recruit) {
            hs::RecruitRaw rr;
            rr.n_windows = W; rr.win_contig = h.win_contig.data(); rr.win_start = h.win_start.data(); rr.win_end = h.win_end.data();
            rr.win_snp_first = raw.win_snp_first; rr.win_snp_last = raw.win_snp_last;
            rr.win_row_off = (const int64_t*)(hr + at.win_row_off); rr.rows = (const hs_recruit_row*)hr;
            rr.contig_base = h.contig_base; rr.params = *recruit;
            if (*(const int32_t*)(hr + at.status) != 0) err = "recruit table: the rows or counters did not fit their arrays";
            else out.recruit.reset(hs::recruit_assemble(rr, err));
            if (!out.recruit) { set_error(err); return HS_EINVAL; }
            float ms_a = 0, ms_b = 0;
            if (ev_rplan.ms(&ms_a) || ev_rrows.ms(&ms_b)) return HS_EHIP;
            out.recruit->t_kernel_ms = (double)ms_a + ms_b; out.recruit->n_counter_words = n_ctr; out.recruit->n_entries = h.n_entries;
        }
        return HS_OK;
    }
};

static int alleles_on_device(const AlleleHostIn& h, const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const int32_t* d_labels,
                             KernelClock& kc, hipStream_t st, const hs_recruit_params* recruit, TablePair& out) {
    TableCall c{h, recruit, kc, st};
    if (int rc = c.queue_plan(d_col_off, d_col_idx, d_col_code, d_labels)) return rc;
    if (int rc = stream_wait(st)) return rc;
    if (int rc = c.size_buffers()) return rc;
    if (int rc = c.queue_cells()) return rc;
    if (int rc = stream_wait(st)) return rc;
    kc.flush();
    return c.assemble(out);
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
// `recruit`: the thresholds of the recruit table, queued behind the cells and assembled with them (nullptr: the allele table alone).
static int pipeline_group_tables(const hs_sr_result* r, const hs::SrSparseLabels& sp, const hs_cv_result* cv, float rsa, int c0, HipSrOps& ops, const hs_recruit_params* recruit,
                                 TablePair& out) {
    const int C = r->n_contigs;
    AlleleHostIn h;
    h.contig_base = c0;
    const int64_t W = r->win_off[C];
    h.windows_of(r);
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
        out.alleles.reset(hs::alleles_assemble(raw, err));
        if (!out.alleles) { set_error(err); return HS_EINVAL; }
        if (recruit) {      // (no rows either; the table still says how many windows the group has)
            const std::vector<int32_t> none((size_t)W + 1, 0);
            const std::vector<int64_t> row_off((size_t)W + 1, 0);
            hs::RecruitRaw rr;
            rr.n_windows = W; rr.win_contig = h.win_contig.data(); rr.win_start = h.win_start.data(); rr.win_end = h.win_end.data();
            rr.win_snp_first = none.data(); rr.win_snp_last = none.data(); rr.win_row_off = row_off.data(); rr.contig_base = c0; rr.params = *recruit;
            out.recruit.reset(hs::recruit_assemble(rr, err));
            if (!out.recruit) { set_error(err); return HS_EINVAL; }
        }
        return HS_OK;
    }
    DBuf d_labels, d_ro, d_ids, d_lab, d_lo;
    UploadPack pk;
    if (int rc = allele_dense_labels(sp, h.label_off, d_labels, pk, d_ro, d_ids, d_lab, d_lo, ops.stream)) return rc;
    return alleles_on_device(h, ops.d_col_off.as<int64_t>(), ops.d_col_idx.as<int32_t>(), ops.d_col_code.as<uint8_t>(), d_labels.as<int32_t>(), ops.kc, ops.stream, recruit, out);
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

// (hs_recruit_reads of hs_capi_recruit.inc is the same call with thresholds and a second table)
static int haplotype_tables(const hs_sr_contig* contigs, int32_t n_contigs, const hs_sr_result* sr, hs_allele_table** table, const hs_recruit_params* recruit,
                            hs_recruit_table** recruit_table) {
    if (int rc = require_device()) return rc;
    if (!contigs || !sr || !table || n_contigs < 0 || sr->n_contigs != n_contigs) { set_error("hs_haplotype_alleles: the result does not describe these contigs"); return HS_EINVAL; }
    if (!sr->labels && sr->win_off[n_contigs] > 0 && sr->label_off[sr->win_off[n_contigs]] > 0) { set_error("hs_haplotype_alleles: the result has no dense labels"); return HS_EINVAL; }
    AlleleHostIn h;
    h.windows_of(sr);
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
    TablePair t;
    if (int rc = alleles_on_device(h, d_co.as<int64_t>(), d_ci.as<int32_t>(), d_cc.as<uint8_t>(), d_labels.as<int32_t>(), kc, st, recruit, t)) return rc;
    *table = t.alleles.release();
    if (recruit) *recruit_table = t.recruit.release();
    return HS_OK;
}

int hs_haplotype_alleles(const hs_sr_contig* contigs, int32_t n_contigs, const hs_sr_result* sr, hs_allele_table** table) {
    return haplotype_tables(contigs, n_contigs, sr, table, nullptr, nullptr);
}

}  // extern "C"
