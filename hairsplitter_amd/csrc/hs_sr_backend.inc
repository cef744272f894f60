// hs_sr_backend.inc -- part of hs_capi.hip: stage 4 on the device. GraphRows (K6 in two halves: one CSR over all (window, masked read)
// rows) and HipSrOps, the HIP implementation of hs::SrDeviceOps: SNP planes + sim / diff, window masks, graphs, the Chinese-Whispers
// chain and the window tails.
// ---------------------------------------------------------------------------------------------------
// stage 4 on the device: every clustering window in its local index space (hs_driver.h: SrWindowSet)
// ---------------------------------------------------------------------------------------------------
// The read graphs of a call: ONE CSR over the rows (window, masked read) with local neighbour ids, the visiting order of
// every window, and the window tables the clustering kernels index. Built by K6 from the resident sim / diff matrices (the
// few rows whose result depends on std::sort's arrangement of equal distances are resolved on the host and patched in) plus
// the rows a caller brings for windows on the low-memory path.
struct GraphRows {
    DBuf d_oo, d_n, d_wc, d_row0, d_ids, d_rw, d_bo, d_fe, d_rank, d_rank_off, d_pos_rank;   // views into `pack`
    bool by_pos = false;      // the contigs' matrices are in the order of the reads' start positions (ws.pos_rank)
    UploadPack pack;
    DBuf d_off, d_nbr, d_visit, d_visit_n, d_prog_info, d_prog_bytes, d_prog_steps, d_prog_adj;
    int64_t rows = 0, rows_dev = 0, total = 0;      // total: neighbour entries of the CSR -- an upper bound while !total_exact (the exact number is d_off[rows])
    bool total_exact = true;
    int W = 0, max_m = 1;
    std::vector<int32_t> win_m;    // [W]
    // what the build leaves behind on the stream: the object keeps it until it dies (or builds again), so that no host wait is needed
    // just to give temporaries back to the pool
    DBuf d_bits, d_amb, d_deg, d_scan, d_wmo, d_ltw, d_lti, d_ltj, d_wsim, d_wdiff, d_stage, d_src, d_len, d_dst, d_os, d_od, d_pb, d_pm, d_pi, d_pj;
    UploadPack pk_amb, pk_patch;
    HBuf h_amb, h_rows, h_deg, h_nbr;
    std::vector<int32_t> row_win;
    std::vector<int64_t> win_bits_off, win_mat_off;
    std::vector<int32_t> lt_w, lt_i, lt_j;
    int Wd = 0, Wmx = 0, rows_mx = 0;
    int row_waves = 0; int64_t n_late = 0;      // wavefronts per workgroup of the row kernels (0: none launched); undecided rows of the last end() fetched behind them
    size_t amb_cap = 0;
    int64_t stage_cap = 0, stage_hint = 0;      // entries (sim / diff pairs) the undecided rows may stage / staged last time
    EventPair ev;
    bool timed = false, begun = false;
    const int32_t* d_sim = nullptr; const int32_t* d_diff = nullptr; int es = 1;
    std::vector<int64_t> ctg_out_off; std::vector<int32_t> ctg_n;
    float* k_ms = nullptr;
};

// the bit rows of the call (K5a), for the windows of the low-memory path
struct PlaneRows { const uint64_t* d_alt = nullptr; const uint64_t* d_ref = nullptr; const int64_t* d_plane_off = nullptr; const int32_t* d_words = nullptr; };

// K6 in two halves. begin: the window tables go up, the row kernels run and -- in the same pass -- stage the sim / diff entries of the
// rows they cannot decide; count, list and staged entries are shipped to pinned memory. Nothing is waited for: the caller has host
// work of its own to do meanwhile (the Chinese-Whispers chain of the call is planned from the window plans alone).
static int graph_rows_begin(const int32_t* d_sim, const int32_t* d_diff, const std::vector<int64_t>& ctg_out_off, const std::vector<int32_t>& ctg_n_matrix,
                            const hs::SrWindowSet& ws, GraphRows& G, hipStream_t stream, float* k_ms, KernelClock* kc = nullptr,
                            const PlaneRows* planes = nullptr, int es = 1 /* element stride of d_sim / d_diff (2: pairs in one array) */) {
    G.ctg_n = ws.ctg_reads.empty() ? ctg_n_matrix : ws.ctg_reads;      // reads of every contig (the matrix list has 0 for low-memory contigs)
    G.ctg_out_off = ctg_out_off;
    const std::vector<int32_t>& ctg_n = G.ctg_n;
    const int W = (int)ws.win_contig.size();
    G.W = W; G.rows = ws.rows(); G.total = 0; G.total_exact = true; G.max_m = 1; G.begun = true; G.timed = false; G.k_ms = k_ms;
    G.d_sim = d_sim; G.d_diff = d_diff; G.es = es; G.row_waves = 0; G.n_late = 0;
    if (G.rows > 0x7fffffff) { set_error("read graphs: too many rows"); return HS_EINVAL; }
    const int rows = (int)G.rows;
    const int Wd = ws.n_dev_windows;
    const int Wmx = ws.ctg_reads.empty() ? Wd : ws.n_matrix_windows;      // [0, Wmx): sim / diff of the contig; [Wmx, Wd): window-local matrices (low-memory path)
    const int rows_dev = (int)ws.win_row0[(size_t)Wd];
    const int rows_mx = (int)ws.win_row0[(size_t)Wmx];
    G.rows_dev = rows_dev; G.Wd = Wd; G.Wmx = Wmx; G.rows_mx = rows_mx;
    if (Wmx < Wd && (!planes || !planes->d_alt)) { set_error("read graphs: low-memory windows without bit rows"); return HS_EINVAL; }
    if ((int64_t)ws.host_off.size() != (int64_t)(rows - rows_dev) + 1 && rows != rows_dev) { set_error("read graphs: host rows do not match the window set"); return HS_EINVAL; }
    std::vector<int32_t>& row_win = G.row_win; row_win.assign((size_t)rows_dev, 0);
    std::vector<int64_t>& win_bits_off = G.win_bits_off; win_bits_off.assign((size_t)Wd + 1, 0);
    G.win_m.resize((size_t)W);
    int max_m_dev = 1, max_len = 1;
    for (int w = 0; w < W; ++w) {
        const int64_t m0 = ws.win_row0[(size_t)w], m = ws.win_row0[(size_t)w + 1] - m0;
        G.win_m[(size_t)w] = (int32_t)m;
        G.max_m = std::max(G.max_m, (int)m);
        if (w < Wd) {
            for (int64_t r = 0; r < m; ++r) row_win[(size_t)(m0 + r)] = w;
            win_bits_off[(size_t)w + 1] = win_bits_off[(size_t)w] + m * ((m + 63) >> 6);
            max_m_dev = std::max(max_m_dev, (int)m);
            max_len = std::max(max_len, w < Wmx ? ctg_n[(size_t)ws.win_contig[(size_t)w]] : (int)m);
        }
    }
    // low-memory windows: an m x m sim / diff per window, every 64 x 64 tile of it one workgroup
    std::vector<int64_t>& win_mat_off = G.win_mat_off; win_mat_off.assign((size_t)Wd + 1, 0);
    std::vector<int32_t>& lt_w = G.lt_w; std::vector<int32_t>& lt_i = G.lt_i; std::vector<int32_t>& lt_j = G.lt_j;
    lt_w.clear(); lt_i.clear(); lt_j.clear();
    for (int w = 0; w < Wd; ++w) {
        const int64_t m = w >= Wmx ? G.win_m[(size_t)w] : 0;
        win_mat_off[(size_t)w + 1] = win_mat_off[(size_t)w] + m * m;
        const int nt = (int)((m + 63) / 64);
        for (int i = 0; i < nt; ++i) for (int j = 0; j < nt; ++j) { lt_w.push_back(w); lt_i.push_back(i); lt_j.push_back(j); }
    }
    if (Wmx < Wd) { G.pack.add(win_mat_off, G.d_wmo); G.pack.add(lt_w, G.d_ltw); G.pack.add(lt_i, G.d_lti); G.pack.add(lt_j, G.d_ltj); }
    G.pack.add(ctg_out_off, G.d_oo);
    G.pack.add(ctg_n, G.d_n);
    G.pack.add(ws.win_contig, G.d_wc);
    G.pack.add(ws.win_row0, G.d_row0);
    G.pack.add(ws.mask_ids, G.d_ids);
    G.pack.add(row_win, G.d_rw);
    G.pack.add(win_bits_off, G.d_bo);
    G.pack.add(ws.win_final_empty, G.d_fe);
    G.pack.add(ws.rank, G.d_rank);
    G.pack.add(ws.ctg_rank_off, G.d_rank_off);
    G.by_pos = !ws.pos_rank.empty();
    if (G.by_pos) G.pack.add(ws.pos_rank, G.d_pos_rank);
    if (int rc = G.pack.commit(stream)) return rc;
    if (int rc = G.d_off.alloc(((size_t)rows + 1) * 8 + 32)) return rc;      // (+ room for the 16-byte granules of a shipment of its last element)
    if (int rc = G.d_visit.alloc(std::max<size_t>((size_t)rows, 1) * 4)) return rc;
    if (int rc = G.d_visit_n.alloc(std::max<size_t>((size_t)W, 1) * 4)) return rc;
    if (rows == 0) { hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, G.d_off.as<uint4>(), 1ll, 0u); HS_HIP(hipGetLastError()); return HS_OK; }
    if (int rc = G.d_deg.alloc((size_t)rows * 4)) return rc;
    if (int rc = G.ev.init()) return rc;
    if (rows_dev > 0) {
        if (rows_mx > 0 && !d_sim) { set_error("read graphs before simdiff"); return HS_EINVAL; }
        const size_t bits_bytes = ((size_t)win_bits_off.back() * 8 + 15) & ~(size_t)15;
        if (int rc = G.d_bits.alloc(std::max<size_t>(bits_bytes, 16))) return rc;
        // the block the host reads: [rows left to it][entries staged] | rows [amb_cap] | stage offsets [amb_cap] ; then the staged entries
        G.amb_cap = (size_t)rows_dev;
        G.stage_cap = std::max<int64_t>(G.stage_hint + G.stage_hint / 2, 64 * (int64_t)max_len);
        const size_t amb_bytes = 16 + (((size_t)G.amb_cap * 4 + 15) & ~(size_t)15) + (((size_t)G.amb_cap * 8 + 15) & ~(size_t)15);      // (every part a whole number of 16-byte granules: the parts of a shipment must not share one)
        if (int rc = G.d_amb.alloc(amb_bytes)) return rc;
        if (int rc = G.d_stage.alloc((size_t)G.stage_cap * 8 + 32)) return rc;
        hipLaunchKernelGGL(hsdev::k_fill16, dim3((unsigned)std::min<size_t>(256, bits_bytes / 4096 + 1)), dim3(256), 0, stream, G.d_bits.as<uint4>(), (long long)(std::max<size_t>(bits_bytes, 16) / 16), 0u);
        hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, G.d_amb.as<uint4>(), 1ll, 0u);
        unsigned long long* amb_head = G.d_amb.as<unsigned long long>();
        int32_t* amb_rows = reinterpret_cast<int32_t*>((char*)G.d_amb.p + 16);
        long long* amb_so = reinterpret_cast<long long*>((char*)G.d_amb.p + 16 + (((size_t)G.amb_cap * 4 + 15) & ~(size_t)15));
        int32_t* st_sim = G.d_stage.as<int32_t>(); int32_t* st_diff = st_sim + (((size_t)G.stage_cap + 3) & ~(size_t)3);
        // per-wave LDS: cap distances + cap totals. Four waves per workgroup while they fit, else one; windows wider than that
        // (m > 7168 masked reads) send their rows to the host
        int cap = ((max_m_dev + 63) / 64) * 64, waves = 4;
        if ((size_t)cap * 8 * 4 > 57344) waves = 1;
        if ((size_t)cap * 8 > 57344) cap = 7168;
        const float below = 1 - ws.error_rate * 2;   // :778
        G.row_waves = waves;
        HS_HIP(ev_rec(G.ev.a, stream));
        if (rows_mx > 0) {
            if (kc) { if (int rc = kc->begin(HS_K_GRAPH_ROWS, stream)) return rc; }
            hipLaunchKernelGGL(hsdev::k_read_graph_rows<false>, dim3((rows_mx + waves - 1) / waves), dim3(64 * waves), (size_t)cap * 8 * waves, stream, d_sim, d_diff,
                               G.d_oo.as<int64_t>(), G.d_n.as<int32_t>(), G.d_wc.as<int32_t>(), G.d_row0.as<int64_t>(), G.d_ids.as<int32_t>(), G.d_rw.as<int32_t>(),
                               G.d_bo.as<int64_t>(), 0, rows_mx, below, cap, G.d_bits.as<unsigned long long>(), amb_head, amb_rows, (int)G.amb_cap,
                               (const int64_t*)nullptr, es, amb_so, st_sim, st_diff, (long long)G.stage_cap, G.by_pos ? G.d_pos_rank.as<int32_t>() : nullptr, G.d_rank_off.as<int64_t>());
            HS_HIP(hipGetLastError());
            if (kc) {   // per row: the sim and diff entries of the window's m reads in, m link bits out
                int64_t by = 0;
                for (int w = 0; w < Wmx; ++w) { const int64_t m = G.win_m[(size_t)w]; by += m * (8 * m + (m + 7) / 8); }
                if (int rc = kc->end(by, stream)) return rc;
            }
        }
        if (rows_dev > rows_mx) {
            // create_read_graph_low_memory: the window-local matrices from the bit rows, then the same row kernel with that path's distance
            const size_t mat = (size_t)win_mat_off.back();
            if (int rc = G.d_wsim.alloc(std::max<size_t>(mat, 1) * 8)) return rc;      // (sim, diff) pairs: a row kernel's two reads of a pair share a line
            G.d_wdiff.release(); G.d_wdiff.p = (char*)G.d_wsim.p + 4; G.d_wdiff.bytes = 0; G.d_wdiff.cap = 0; G.d_wdiff.view = true;
            if (kc) { if (int rc = kc->begin(HS_K_SIMDIFF, stream)) return rc; }
            hipLaunchKernelGGL(hsdev::k_simdiff_windows, dim3((unsigned)lt_w.size()), dim3(256), 0, stream, planes->d_alt, planes->d_ref, planes->d_plane_off, planes->d_words,
                               G.d_wc.as<int32_t>(), G.d_row0.as<int64_t>(), G.d_ids.as<int32_t>(), G.d_wmo.as<int64_t>(), G.d_ltw.as<int32_t>(), G.d_lti.as<int32_t>(),
                               G.d_ltj.as<int32_t>(), G.d_wsim.as<int32_t>(), G.d_wdiff.as<int32_t>(), 2);
            HS_HIP(hipGetLastError());
            if (kc) { if (int rc = kc->end(8 * (int64_t)mat, stream)) return rc; }
            if (kc) { if (int rc = kc->begin(HS_K_GRAPH_ROWS, stream)) return rc; }
            const int n_lm = rows_dev - rows_mx;
            hipLaunchKernelGGL(hsdev::k_read_graph_rows<true>, dim3((n_lm + waves - 1) / waves), dim3(64 * waves), (size_t)cap * 8 * waves, stream, G.d_wsim.as<int32_t>(),
                               G.d_wdiff.as<int32_t>(), G.d_oo.as<int64_t>(), G.d_n.as<int32_t>(), G.d_wc.as<int32_t>(), G.d_row0.as<int64_t>(), G.d_ids.as<int32_t>(),
                               G.d_rw.as<int32_t>(), G.d_bo.as<int64_t>(), rows_mx, n_lm, below, cap, G.d_bits.as<unsigned long long>(), amb_head, amb_rows, (int)G.amb_cap,
                               G.d_wmo.as<int64_t>(), 2, amb_so, st_sim, st_diff, (long long)G.stage_cap, (const int32_t*)nullptr, (const int64_t*)nullptr);
            HS_HIP(hipGetLastError());
            if (kc) { if (int rc = kc->end(8 * (int64_t)mat, stream)) return rc; }
        }
        HS_HIP(ev_rec(G.ev.b, stream));
        G.timed = true;
        // count, list, stage offsets and the staged entries in one shipment
        const size_t rows_part = ((size_t)G.amb_cap * 4 + 15) & ~(size_t)15, stage_half = (((size_t)G.stage_cap + 3) & ~(size_t)3) * 4;
        if (int rc = G.h_amb.alloc(amb_bytes + 2 * stage_half + 64)) return rc;
        Shipment sh;
        char* hb = (char*)G.h_amb.p;
        sh.add(hb, G.d_amb.p, 16);
        sh.add_counted(hb + 16, (char*)G.d_amb.p + 16, reinterpret_cast<const long long*>(amb_head), 4, (long long)G.amb_cap);
        sh.add_counted(hb + 16 + rows_part, (char*)G.d_amb.p + 16 + rows_part, reinterpret_cast<const long long*>(amb_head), 8, (long long)G.amb_cap);
        sh.add_counted(hb + amb_bytes, st_sim, reinterpret_cast<const long long*>(amb_head + 1), 4, G.stage_cap);
        sh.add_counted(hb + amb_bytes + stage_half, st_diff, reinterpret_cast<const long long*>(amb_head + 1), 4, G.stage_cap);
        if (kc) { if (int rc = kc->begin(HS_K_SHIP, stream)) return rc; }
        if (int rc = sh.launch(stream, 16)) return rc;
        if (kc) { if (int rc = kc->end(0, stream)) return rc; }
    }
    return HS_OK;
}

// end: the one wait of K6; the undecided rows are resolved with std::sort itself on the staged entries and patched in; degrees, scan,
// fill (the neighbour array sized by its upper bound sum m^2 where that is moderate: no round trip for the total), visiting orders.
// Nothing is waited for at the end: what the stream still reads lives in G.
static int graph_rows_end(const hs::SrWindowSet& ws, GraphRows& G, hipStream_t stream, int64_t* rows_on_host, KernelClock* kc = nullptr) {
    if (rows_on_host) *rows_on_host = 0;
    const int rows = (int)G.rows, rows_dev = (int)G.rows_dev, rows_mx = G.rows_mx, Wd = G.Wd, Wmx = G.Wmx, W = G.W;
    if (rows == 0) return HS_OK;
    const std::vector<int32_t>& ctg_n = G.ctg_n;
    const std::vector<int32_t>& row_win = G.row_win;
    const std::vector<int64_t>& win_bits_off = G.win_bits_off;
    const std::vector<int64_t>& win_mat_off = G.win_mat_off;
    if (rows_dev > 0) {
        if (int rc = stream_wait(stream)) return rc;
        const size_t rows_part = ((size_t)G.amb_cap * 4 + 15) & ~(size_t)15, amb_bytes = 16 + rows_part + (((size_t)G.amb_cap * 8 + 15) & ~(size_t)15), stage_half = (((size_t)G.stage_cap + 3) & ~(size_t)3) * 4;
        const char* hb = (const char*)G.h_amb.p;
        const int64_t n_amb = (int64_t)((const unsigned long long*)hb)[0];
        const int64_t staged = (int64_t)((const unsigned long long*)hb)[1];
        G.stage_hint = staged;
        if (n_amb > (int64_t)G.amb_cap) { set_error("read graphs: more undecided rows than rows"); return HS_EINVAL; }
        if (n_amb > 0) {
            // rows where std::sort's arrangement of equal distances decides: exactly what the reference does, on their sim / diff entries
            const int32_t* amb_rows = (const int32_t*)(hb + 16);
            const long long* amb_so = (const long long*)(hb + 16 + rows_part);
            const int32_t* st_sim = (const int32_t*)(hb + amb_bytes); const int32_t* st_diff = (const int32_t*)(hb + amb_bytes + stage_half);
            std::vector<int32_t> order((size_t)n_amb);
            for (int64_t k = 0; k < n_amb; ++k) order[(size_t)k] = (int32_t)k;
            std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return amb_rows[x] < amb_rows[y]; });      // (the links are ORed in: any order gives the same bits; sorted for the fetch below)
            // rows whose entries found no room in the staging area (a first call, or more of them than ever before): fetched the old way
            std::vector<int32_t> late;
            for (int32_t k : order) if (amb_so[k] < 0) late.push_back(k);
            G.n_late = (int64_t)late.size();
            std::vector<int64_t> late_dst((size_t)late.size() + 1, 0);
            const int32_t* late_sim = nullptr; const int32_t* late_diff = nullptr;
            if (!late.empty()) {
                std::vector<int64_t> src(late.size()); std::vector<int32_t> len(late.size());
                int n_mx = 0;
                for (size_t q = 0; q < late.size(); ++q) {
                    const int row = amb_rows[late[q]];
                    const int w = row_win[(size_t)row];
                    const int c = ws.win_contig[(size_t)w];
                    const int N = ctg_n[(size_t)c];
                    const int r1 = ws.mask_ids[(size_t)row];
                    if (row < rows_mx) { const int r1k = G.by_pos ? ws.pos_rank[(size_t)ws.ctg_rank_off[(size_t)c] + (size_t)r1] : r1; src[q] = G.ctg_out_off[(size_t)c] + (int64_t)r1k * N; len[q] = N; n_mx++; }
                    else { const int64_t m = G.win_m[(size_t)w]; src[q] = win_mat_off[(size_t)w] + (int64_t)(row - ws.win_row0[(size_t)w]) * m; len[q] = (int32_t)m; }
                    late_dst[q + 1] = late_dst[q] + len[q];
                }
                G.pk_amb.add(src, G.d_src); G.pk_amb.add(len, G.d_len); G.pk_amb.add(late_dst, G.d_dst);
                if (int rc = G.pk_amb.commit(stream)) return rc;
                if (int rc = G.d_os.alloc((size_t)late_dst.back() * 4 + 16)) return rc;
                if (int rc = G.d_od.alloc((size_t)late_dst.back() * 4 + 16)) return rc;
                if (n_mx > 0)
                    hipLaunchKernelGGL(hsdev::k_read_graph_fetch_rows, dim3(n_mx), dim3(256), 0, stream, G.d_sim, G.d_diff, G.d_src.as<int64_t>(), G.d_len.as<int32_t>(),
                                       G.d_dst.as<int64_t>(), G.d_os.as<int32_t>(), G.d_od.as<int32_t>(), G.es);
                if ((int)late.size() > n_mx)
                    hipLaunchKernelGGL(hsdev::k_read_graph_fetch_rows, dim3((unsigned)late.size() - n_mx), dim3(256), 0, stream, G.d_wsim.as<int32_t>(), G.d_wdiff.as<int32_t>(),
                                       G.d_src.as<int64_t>() + n_mx, G.d_len.as<int32_t>() + n_mx, G.d_dst.as<int64_t>() + n_mx, G.d_os.as<int32_t>(), G.d_od.as<int32_t>(), 2);
                HS_HIP(hipGetLastError());
                const size_t row_bytes = (((size_t)late_dst.back() * 4) + 15) & ~(size_t)15;
                if (int rc = G.h_rows.alloc(2 * row_bytes + 16)) return rc;
                Shipment sh; sh.add(G.h_rows.p, G.d_os.p, row_bytes); sh.add((char*)G.h_rows.p + row_bytes, G.d_od.p, row_bytes);
                if (int rc = sh.launch(stream, 16)) return rc;
                if (int rc_w = stream_wait(stream)) return rc_w;
                late_sim = (const int32_t*)G.h_rows.p; late_diff = (const int32_t*)((const char*)G.h_rows.p + row_bytes);
                G.stage_hint = std::max<int64_t>(G.stage_hint, staged + late_dst.back());
            }
            std::vector<int64_t> pbase; std::vector<int32_t> pmw, pi, pj;
            std::vector<uint8_t> mask;
            std::vector<int> picked;
            size_t late_q = 0;
            for (int32_t k : order) {
                const int row = amb_rows[k];
                const int w = row_win[(size_t)row];
                const int64_t m0 = ws.win_row0[(size_t)w];
                const int m = (int)(ws.win_row0[(size_t)w + 1] - m0);
                const int32_t* ids = ws.mask_ids.data() + m0;
                const int N = ctg_n[(size_t)ws.win_contig[(size_t)w]];
                const int32_t* rs; const int32_t* rd;
                std::vector<int32_t> perm_s, perm_d;
                if (late_q < late.size() && late[late_q] == k) {
                    rs = late_sim + late_dst[late_q]; rd = late_diff + late_dst[late_q]; late_q++;
                    if (G.by_pos && row < rows_mx) {      // (fetched as the matrix has the row: by position rank -- the host walks it by read)
                        const int32_t* pr = ws.pos_rank.data() + ws.ctg_rank_off[(size_t)ws.win_contig[(size_t)w]];
                        perm_s.resize((size_t)N); perm_d.resize((size_t)N);
                        for (int r = 0; r < N; ++r) { perm_s[(size_t)r] = rs[pr[r]]; perm_d[(size_t)r] = rd[pr[r]]; }
                        rs = perm_s.data(); rd = perm_d.data();
                    }
                }
                else { rs = st_sim + amb_so[k]; rd = st_diff + amb_so[k]; }
                mask.assign((size_t)N, 0);
                for (int j = 0; j < m; ++j) mask[(size_t)ids[j]] = 1;
                if (row < rows_mx) hs::sr_pick_row_sorted(rs, rd, N, ids[row - m0], mask.data(), ws.error_rate, picked);
                else hs::sr_pick_row_sorted_low_memory(rs, rd, ids, m, (int)(row - m0), N, mask.data(), ws.error_rate, picked);
                for (int nb : picked) {
                    const int j = (int)(std::lower_bound(ids, ids + m, nb) - ids);
                    pbase.push_back(win_bits_off[(size_t)w]); pmw.push_back((m + 63) >> 6); pi.push_back((int32_t)(row - m0)); pj.push_back(j);
                }
            }
            if (!pi.empty()) {
                G.pk_patch.add(pbase, G.d_pb); G.pk_patch.add(pmw, G.d_pm); G.pk_patch.add(pi, G.d_pi); G.pk_patch.add(pj, G.d_pj);
                if (int rc = G.pk_patch.commit(stream)) return rc;
                const int np = (int)pi.size();
                hipLaunchKernelGGL(hsdev::k_read_graph_patch, dim3((np + 255) / 256), dim3(256), 0, stream, G.d_pb.as<int64_t>(), G.d_pm.as<int32_t>(), G.d_pi.as<int32_t>(),
                                   G.d_pj.as<int32_t>(), np, G.d_bits.as<unsigned long long>());
                HS_HIP(hipGetLastError());
            }
            if (rows_on_host) *rows_on_host = n_amb;
            if (std::getenv("HS_TIMING") && Wmx < Wd) {
                int64_t n_lm = 0; for (int64_t k = 0; k < n_amb; ++k) n_lm += amb_rows[k] >= rows_mx;
                std::fprintf(stderr, "[hs timing] sr: low-memory path on the device: %d windows, %d rows, %ld of them resolved on the host (NaN distances / std::sort ties)\n",
                             Wd - Wmx, rows_dev - rows_mx, (long)n_lm);
            }
        } else if (std::getenv("HS_TIMING") && Wmx < Wd)
            std::fprintf(stderr, "[hs timing] sr: low-memory path on the device: %d windows, %d rows, none resolved on the host\n", Wd - Wmx, rows_dev - rows_mx);
        if (kc) { if (int rc = kc->begin(HS_K_GRAPH_CSR, stream)) return rc; }
        hipLaunchKernelGGL(hsdev::k_read_graph_degrees, dim3((rows_dev + 255) / 256), dim3(256), 0, stream, G.d_bits.as<unsigned long long>(), G.d_rw.as<int32_t>(),
                           G.d_row0.as<int64_t>(), G.d_bo.as<int64_t>(), rows_dev, G.d_deg.as<int32_t>());
        HS_HIP(hipGetLastError());
        if (kc) { if (int rc = kc->end((int64_t)win_bits_off.back() * 8 + 4 * (int64_t)rows_dev, stream)) return rc; }
    }
    if (rows > rows_dev) {   // degrees of the rows the host brings
        const size_t nh = (size_t)(rows - rows_dev);
        if (int rc = G.h_deg.alloc(nh * 4 + 16)) return rc;
        int32_t* hd = (int32_t*)G.h_deg.p;
        for (size_t r = 0; r < nh; ++r) hd[r] = (int32_t)(ws.host_off[r + 1] - ws.host_off[r]);
        HS_HIP(HS_COPY_ASYNC(G.d_deg.as<int32_t>() + rows_dev, hd, nh * 4, hipMemcpyHostToDevice, stream));
    }
    if (int rc = exclusive_scan_launch(G.d_deg.as<int32_t>(), rows, G.d_off.as<int64_t>(), G.d_scan, stream)) return rc;
    // the neighbour array: at most sum m^2 entries for the device rows; the exact number only has to be known here when host rows have to
    // be placed behind them (contigs whose low-memory graphs the host builds) or when the bound is unreasonable
    int64_t bound = (int64_t)ws.host_nbr.size();
    for (int w = 0; w < Wd; ++w) bound += (int64_t)G.win_m[(size_t)w] * G.win_m[(size_t)w];
    int64_t total = bound;
    G.total_exact = false;
    if (!ws.host_nbr.empty() || bound > ((int64_t)1 << 28)) {
        if (int rc = d2h_pinned(&total, G.d_off.as<int64_t>() + rows, 8, stream)) return rc;
        G.total_exact = true;
    }
    G.total = total;
    if (int rc = G.d_nbr.alloc(std::max<size_t>((size_t)total, 1) * 4)) return rc;
    if (total > 0) {
        if (rows_dev > 0) {
            if (kc) { if (int rc = kc->begin(HS_K_GRAPH_CSR, stream)) return rc; }
            hipLaunchKernelGGL(hsdev::k_read_graph_fill, dim3((rows_dev + 255) / 256), dim3(256), 0, stream, G.d_bits.as<unsigned long long>(), G.d_rw.as<int32_t>(),
                               G.d_row0.as<int64_t>(), G.d_bo.as<int64_t>(), G.d_off.as<int64_t>(), rows_dev, G.d_nbr.as<int32_t>());
            HS_HIP(hipGetLastError());
            if (kc) { if (int rc = kc->end((int64_t)win_bits_off.back() * 8 + 4 * (G.total_exact ? total : (int64_t)rows_dev * 20), stream)) return rc; }
        }
        if (!ws.host_nbr.empty()) {   // the host rows sit behind the device rows: their lists start at total - |host_nbr|
            const size_t nb = ws.host_nbr.size() * 4;
            if (int rc = G.h_nbr.alloc(nb)) return rc;
            std::memcpy(G.h_nbr.p, ws.host_nbr.data(), nb);
            HS_HIP(HS_COPY_ASYNC(G.d_nbr.as<int32_t>() + (total - (int64_t)ws.host_nbr.size()), G.h_nbr.p, nb, hipMemcpyHostToDevice, stream));
        }
    }
    {   // visiting order of every window (hs_kernels_cw.hip)
        const int cap = std::min(((G.max_m + 63) / 64) * 64, 8192);
        // the visit programs of the row-packed Chinese-Whispers kernel (windows with m <= 255): nnz + 15 m bytes per window
        if (int rc = G.d_prog_info.alloc(std::max<size_t>((size_t)rows, 1) * 4)) return rc;
        if (int rc = G.d_prog_bytes.alloc((size_t)total + 15 * (size_t)rows + 64)) return rc;
        const size_t steps_bytes = (std::max<size_t>((size_t)W, 1) * 4 + 15) & ~(size_t)15;
        if (int rc = G.d_prog_steps.alloc(steps_bytes)) return rc;
        if (int rc = G.d_prog_adj.alloc(std::max<size_t>((size_t)rows, 1) * 8)) return rc;
        hipLaunchKernelGGL(hsdev::k_fill16, dim3((unsigned)std::min<size_t>(64, steps_bytes / 4096 + 1)), dim3(256), 0, stream, G.d_prog_steps.as<uint4>(), (long long)(steps_bytes / 16), 0u);
        if (kc) { if (int rc = kc->begin(HS_K_VISIT_LISTS, stream)) return rc; }
        hipLaunchKernelGGL(hsdev::k_cw_visit_lists, dim3((unsigned)W), dim3(256), (size_t)cap * 4, stream, G.d_off.as<int64_t>(), G.d_nbr.as<int32_t>(), G.d_row0.as<int64_t>(),
                           G.d_ids.as<int32_t>(), G.d_wc.as<int32_t>(), G.d_rank_off.as<int64_t>(), G.d_rank.as<int32_t>(), W, cap, G.d_visit.as<int32_t>(),
                           G.d_visit_n.as<int32_t>(), G.d_prog_info.as<uint32_t>(), G.d_prog_bytes.as<uint8_t>(), G.d_prog_steps.as<int32_t>(),
                           G.d_prog_adj.as<unsigned long long>());
        HS_HIP(hipGetLastError());
        if (kc) { if (int rc = kc->end(20 * (int64_t)rows, stream)) return rc; }   // row offsets + read id + rank in, visiting slot out
    }
    return HS_OK;
}
// after a wait of the stream: the kernel clocks and the K6 time of the call
static int graph_rows_settle(GraphRows& G, KernelClock* kc) {
    if (kc) kc->flush();
    if (G.timed) { G.timed = false; float m = 0; if (int rc = G.ev.ms(&m)) return rc; if (G.k_ms) *G.k_ms += m; }
    return HS_OK;
}
// both halves and a wait: the graphs are complete and G.total is their exact size (the kernel-level entry point)
static int graph_rows_build(const int32_t* d_sim, const int32_t* d_diff, const std::vector<int64_t>& ctg_out_off, const std::vector<int32_t>& ctg_n_matrix,
                            const hs::SrWindowSet& ws, GraphRows& G, hipStream_t stream, int64_t* rows_on_host, float* k_ms, KernelClock* kc = nullptr,
                            const PlaneRows* planes = nullptr, int es = 1) {
    if (int rc = graph_rows_begin(d_sim, d_diff, ctg_out_off, ctg_n_matrix, ws, G, stream, k_ms, kc, planes, es)) return rc;
    if (int rc = graph_rows_end(ws, G, stream, rows_on_host, kc)) return rc;
    if (G.rows > 0 && !G.total_exact) { int64_t t = 0; if (int rc = d2h_pinned(&t, G.d_off.as<int64_t>() + G.rows, 8, stream)) return rc; G.total = t; G.total_exact = true; }
    else if (int rc_w = stream_wait(stream)) return rc_w;
    return graph_rows_settle(G, kc);
}

struct HipSrOps : hs::SrDeviceOps {
    hipStream_t stream = nullptr;
    DBuf d_sim, d_diff;                       // K5 results stay in HBM for K6
    std::vector<int64_t> sd_out_off;
    std::vector<int32_t> sd_n;
    GraphRows G;
    KernelClock kc;

    // K5 runs on while the host plans the windows: its temporaries and its timing events are parked here until the next
    // call that waits for the stream anyway
    struct SimdiffInFlight {
        DBuf d_alt, d_ref, d_sr, d_sa, d_sc, d_cb, d_po, d_n, d_pn, d_w, d_oo, t_c, t_i, t_j, d_bc, d_bw, d_rb, d_orig, d_rng;
        std::vector<int32_t> tc, ti, tj, blk_c, blk_w;      // (the lists ride in the one upload of the call)
        UploadPack pk;
        EventPair ev;
        float* k_ms = nullptr;
    };
    std::unique_ptr<SimdiffInFlight> sd_flight;
    int settle_simdiff(bool account = true) {   // waits for K5 if it is still running, accounts its time, releases its temporaries
        if (!sd_flight) return HS_OK;
        float m = 0;
        // (untimed step: no event to wait on; K5 is complete when the stream has been waited for since its launch -- the window masks' wait,
        // the graph rows' -- and only a batch without either has to look at the stream)
        int rc = (sd_flight->ev.a || k5_waited) ? HS_OK : stream_wait_quiet(stream);
        if (!rc) rc = sd_flight->ev.ms(&m);
        if (!rc && account && sd_flight->k_ms) *sd_flight->k_ms += m;
        sd_flight.reset();
        return rc;
    }
    bool k5_waited = false;      // the stream has been waited for since K5 was queued
    ~HipSrOps() override { (void)settle_simdiff(false); }   // the caller's counter may be gone by now

    DBuf d_col_off, d_col_idx, d_col_code;    // SNP columns of the batch: uploaded once (or taken over from stage 3), read by K5a and the seeded CW runs
    UploadPack col_pack;
    const hs::CwChain* resident_cols = nullptr;
    // stage 3 -> 4 on the device: the packed SNP columns HipCvOps::finish_columns left (offsets, read indices, codes) become this
    // object's columns; nothing is uploaded
    bool adopted = false;
    int64_t adopted_cols = 0, adopted_entries = 0;
    DBuf cols_block;      // (adopted: the packed SNP block of stage 3; d_col_off / d_col_idx / d_col_code are views into it)
    void adopt_columns(HipCvOps& cv) {
        std::swap(cols_block, cv.d_pk);
        char* base = (char*)cols_block.p;
        auto view = [&](DBuf& d, size_t off, size_t bytes) { d.release(); d.p = base + off; d.bytes = bytes; d.cap = 0; d.view = true; };
        view(d_col_off, cv.pk_layout.off, ((size_t)cv.snp_count + 1) * 8);
        view(d_col_idx, cv.pk_layout.idx, (size_t)cv.snp_entries * 4);
        view(d_col_code, cv.pk_layout.code, (size_t)cv.snp_entries);
        adopted = true; adopted_cols = cv.snp_count; adopted_entries = cv.snp_entries;
    }
    bool columns_resident() const override { return adopted; }
    // (HS_LOW_MEMORY_GRAPHS_ON_HOST=1: the windows of the low-memory path keep the host builder)
    bool low_memory_graphs() const override { static const bool host = std::getenv("HS_LOW_MEMORY_GRAPHS_ON_HOST") != nullptr; return !host; }
    void drop_resident_columns() override { adopted = false; resident_cols = nullptr; }
    int fetch_columns(std::vector<int32_t>& idx, std::vector<uint8_t>& code) override {
        if (!adopted) { set_error("fetch_columns: no resident columns"); return HS_EINVAL; }
        idx.resize((size_t)adopted_entries); code.resize((size_t)adopted_entries);
        if (adopted_entries == 0) return HS_OK;
        if (int rc = d2h_pinned(idx.data(), d_col_idx.p, (size_t)adopted_entries * 4, stream)) return rc;
        return d2h_pinned(code.data(), d_col_code.p, (size_t)adopted_entries, stream);
    }
    int window_masks(const std::vector<int64_t>& col_a, const std::vector<int64_t>& col_b, const std::vector<int64_t>& slot_off,
                     std::vector<int32_t>& ids, std::vector<int32_t>& win_m) override {
        if (!adopted) { set_error("window_masks: no resident columns"); return HS_EINVAL; }
        const int W = (int)col_a.size();
        const int64_t total = slot_off.back();
        ids.resize((size_t)total); win_m.assign((size_t)W, 0);
        if (W == 0) return HS_OK;
        DBuf d_a, d_b, d_so, d_ids;
        UploadPack pk;
        pk.add(col_a, d_a); pk.add(col_b, d_b); pk.add(slot_off, d_so);
        if (int rc = pk.commit(stream)) return rc;
        // the ids and the per-window counts in one block: one copy back
        const size_t ids_bytes = ((size_t)total * 4 + 255) & ~(size_t)255;
        if (int rc = d_ids.alloc(ids_bytes + (size_t)W * 4 + 16)) return rc;
        int32_t* const dm = reinterpret_cast<int32_t*>((char*)d_ids.p + ids_bytes);
        if (int rc = kc.begin(HS_K_WINDOW_MASKS, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_window_masks, dim3((unsigned)((W + 3) / 4)), dim3(256), 0, stream, d_col_off.as<int64_t>(), d_col_idx.as<int32_t>(), d_a.as<int64_t>(),
                           d_b.as<int64_t>(), d_so.as<int64_t>(), W, d_ids.as<int32_t>(), dm);
        HS_HIP(hipGetLastError());
        if (int rc = kc.end(8 * total + 4 * (int64_t)W, stream)) return rc;
        HBuf h_ids;
        if (int rc = h_ids.alloc(ids_bytes + (size_t)W * 4 + 16)) return rc;
        { Shipment sh; sh.add(h_ids.p, d_ids.p, ids_bytes + (size_t)W * 4); if (int rc = sh.launch(stream, 32)) return rc; }
        if (int rc = stream_wait(stream)) return rc;
        k5_waited = true;
        if (total) std::memcpy(ids.data(), h_ids.p, (size_t)total * 4);
        std::memcpy(win_m.data(), (const char*)h_ids.p + ids_bytes, (size_t)W * 4);
        kc.flush();
        return HS_OK;
    }
    int simdiff_columns(const hs::SimdiffJob& job, float* k_ms) override {
        const hs::CwChain& ch = *job.cols;
        if (!adopted) {
            col_pack.add(ch.col_off, d_col_off); col_pack.add(ch.col_idx, d_col_idx); col_pack.add(ch.col_code, d_col_code);
            if (int rc = col_pack.commit(stream)) return rc;
        } else if ((int64_t)ch.col_off.size() != adopted_cols + 1) { set_error("simdiff_columns: the resident columns are not those of this call"); return HS_EINVAL; }
        resident_cols = job.cols;
        sd_out_off = job.out_off; sd_n = job.n_reads;
        if (job.out_total <= 0 && job.plane_total <= 0) return HS_OK;
        if (int rc = settle_simdiff()) return rc;
        sd_flight.reset(new SimdiffInFlight());
        k5_waited = false;
        SimdiffInFlight& f = *sd_flight;
        f.k_ms = k_ms;
        f.pk.add(job.snp_ref, f.d_sr);
        f.pk.add(job.snp_alt, f.d_sa);
        f.pk.add(job.snp_contig, f.d_sc);
        f.pk.add(job.contig_snp_base, f.d_cb);
        f.pk.add(job.plane_off, f.d_po);
        f.pk.add(job.n_reads, f.d_n);
        f.pk.add(job.plane_n, f.d_pn);
        f.pk.add(job.words, f.d_w);
        f.pk.add(job.out_off, f.d_oo);
        snp_planes_blocks(job.words.data(), (int)job.words.size(), f.blk_c, f.blk_w);
        simdiff_tiles(job.n_reads, f.tc, f.ti, f.tj);
        f.pk.add(f.blk_c, f.d_bc); f.pk.add(f.blk_w, f.d_bw); f.pk.add(f.tc, f.t_c); f.pk.add(f.ti, f.t_i); f.pk.add(f.tj, f.t_j);
        // rows of the matrices in the order of the reads' start positions (the job says so): K5a notes the words every read is present in, K5
        // skips the pairs of 64-read blocks that share none and walks the common words only
        const bool by_pos = !job.pos_orig.empty();
        const size_t rows_all = job.pos_orig.size();
        if (by_pos) { f.pk.add(job.read_base, f.d_rb); f.pk.add(job.pos_orig, f.d_orig); }
        if (int rc = f.pk.commit(stream)) return rc;
        int32_t* rng_lo = nullptr; int32_t* rng_hi = nullptr;
        if (by_pos) {
            const size_t half = ((rows_all * 4 + 15) & ~(size_t)15);
            if (int rc = f.d_rng.alloc(2 * half + 16)) return rc;
            rng_lo = f.d_rng.as<int32_t>(); rng_hi = reinterpret_cast<int32_t*>((char*)f.d_rng.p + half);
            const unsigned gb = (unsigned)std::min<size_t>(64, half / 4096 + 1);
            hipLaunchKernelGGL(hsdev::k_fill16, dim3(gb), dim3(256), 0, stream, reinterpret_cast<uint4*>(rng_lo), (long long)(half / 16), 0x7fffffffu);
            hipLaunchKernelGGL(hsdev::k_fill16, dim3(gb), dim3(256), 0, stream, reinterpret_cast<uint4*>(rng_hi), (long long)(half / 16), 0xffffffffu);
        }
        const size_t pbytes = (size_t)job.plane_total * sizeof(uint64_t);
        const size_t tap_pad = front ? 16 : 0;      // (test taps: room for the whole 16-byte granules of the fills below)
        if (int rc = f.d_alt.alloc(pbytes + tap_pad)) return rc;
        if (int rc = f.d_ref.alloc(pbytes + tap_pad)) return rc;
        // (sim, diff) of a read pair side by side: K6 reads both for every masked read of a row, one 64-byte line instead of two
        if (int rc = d_sim.alloc(std::max<size_t>((size_t)job.out_total, 1) * 2 * sizeof(int32_t) + tap_pad)) return rc;
        d_diff.release(); d_diff.p = (char*)d_sim.p + sizeof(int32_t); d_diff.bytes = 0; d_diff.cap = 0; d_diff.view = true;
        if (front) {      // test taps only: a word K5a does not store stays all ones, an entry K5 does not write stays the sentinel
            auto fill = [&](void* p, size_t bytes, unsigned v) {
                const long long n16 = (long long)((bytes + 15) / 16);
                if (n16) hipLaunchKernelGGL(hsdev::k_fill16, dim3((unsigned)std::min<long long>(256, n16 / 4096 + 1)), dim3(256), 0, stream, reinterpret_cast<uint4*>(p), n16, v);
            };
            fill(f.d_alt.p, pbytes, 0xffffffffu); fill(f.d_ref.p, pbytes, 0xffffffffu);
            fill(d_sim.p, (size_t)job.out_total * 8, (unsigned)hs::SrGraphTaps::kSentinel);
            HS_HIP(hipGetLastError());
        }
        if (int rc = kc.begin(HS_K_SNP_PLANES, stream)) return rc;
        if (int rc = snp_planes_launch(d_col_off.as<int64_t>(), d_col_idx.as<int32_t>(), d_col_code.as<uint8_t>(), f.d_sr.as<uint8_t>(), f.d_sa.as<uint8_t>(),
                                       f.d_sc.as<int32_t>(), f.d_cb.as<int64_t>(), f.d_po.as<int64_t>(), f.d_w.as<int32_t>(), f.d_pn.as<int32_t>(), f.d_bc.as<int32_t>(),
                                       f.d_bw.as<int32_t>(), f.blk_c.size(), (int32_t)job.snp_ref.size(), f.d_alt.as<uint64_t>(), f.d_ref.as<uint64_t>(), stream,
                                       by_pos ? f.d_rb.as<int64_t>() : nullptr, rng_lo, rng_hi)) return rc;
        if (int rc = kc.end(5 * (adopted ? adopted_entries : (int64_t)ch.col_idx.size()) + 2 * (int64_t)pbytes, stream)) return rc;
        if (int rc = f.ev.init()) return rc;
        HS_HIP(ev_rec(f.ev.a, stream));
        if (int rc = kc.begin(HS_K_SIMDIFF, stream)) return rc;
        if (int rc = simdiff_launch(f.d_alt.as<uint64_t>(), f.d_ref.as<uint64_t>(), f.d_po.as<int64_t>(), f.d_n.as<int32_t>(), f.d_w.as<int32_t>(),
                                    f.d_oo.as<int64_t>(), d_sim.as<int32_t>(), d_diff.as<int32_t>(), stream, f.t_c.as<int32_t>(), f.t_i.as<int32_t>(), f.t_j.as<int32_t>(), f.tc.size(), 2,
                                    by_pos ? f.d_rb.as<int64_t>() : nullptr, by_pos ? f.d_orig.as<int32_t>() : nullptr, rng_lo, rng_hi)) return rc;
        if (int rc = kc.end(2 * (int64_t)pbytes + 8 * job.out_total, stream)) return rc;   // the two bit-planes in, sim + diff out
        HS_HIP(ev_rec(f.ev.b, stream));
        if (front) {      // test taps only: bit rows and matrices to the host, as the kernels left them
            front->alt.assign((size_t)job.plane_total, ~0ull); front->ref.assign((size_t)job.plane_total, ~0ull);
            front->matrix.assign((size_t)job.out_total * 2, 0);
            if (pbytes) { if (int rc = d2h_pinned(front->alt.data(), f.d_alt.p, pbytes, stream)) return rc; if (int rc = d2h_pinned(front->ref.data(), f.d_ref.p, pbytes, stream)) return rc; }
            if (job.out_total > 0) { if (int rc = d2h_pinned(front->matrix.data(), d_sim.p, (size_t)job.out_total * 8, stream)) return rc; }
        }
        return HS_OK;   // not waited for: the stream orders K6 behind it, the host goes on planning the windows
    }

    hs::SrGraphTaps* front = nullptr;      // test taps of the front of the call (hs_driver.h), while they are on
    void tap_front(hs::SrGraphTaps* t) override { front = t; }
    struct Keep { int64_t stage_hint = 0; };      // kept by the caller from step to step: how much the undecided graph rows staged
    Keep* keep = nullptr;
    PlaneRows plane_rows() const {
        PlaneRows pr;
        if (sd_flight) { pr.d_alt = sd_flight->d_alt.as<uint64_t>(); pr.d_ref = sd_flight->d_ref.as<uint64_t>(); pr.d_plane_off = sd_flight->d_po.as<int64_t>(); pr.d_words = sd_flight->d_w.as<int32_t>(); }
        return pr;
    }
    int build_graphs(const hs::SrWindowSet& ws, int64_t* rows_on_host, float* k_ms) override {
        if (int rc = build_graphs_begin(ws, k_ms)) return rc;
        return build_graphs_end(ws, rows_on_host);
    }
    bool two_phase_graphs() const override { return true; }
    int build_graphs_begin(const hs::SrWindowSet& ws, float* k_ms) override {
        const PlaneRows pr = plane_rows();
        if (keep) G.stage_hint = keep->stage_hint;
        return graph_rows_begin(d_sim.as<int32_t>(), d_diff.as<int32_t>(), sd_out_off, sd_n, ws, G, stream, k_ms, &kc, &pr, 2);
    }
    int build_graphs_end(const hs::SrWindowSet& ws, int64_t* rows_on_host) override {
        const int rc = graph_rows_end(ws, G, stream, rows_on_host, &kc);
        if (!rc) k5_waited = true;      // (graph_rows_end has waited for the stream)
        if (!rc && front) { front->rows_late = G.n_late; front->row_waves = G.row_waves; }
        if (keep) keep->stage_hint = G.stage_hint;
        return rc;      // (not waited for: K5's temporaries and the clocks are settled behind the wait of cw_chain / the destructor)
    }
    int fetch_graphs(std::vector<int64_t>& off, std::vector<int32_t>& nbr) override {
        if (G.rows > 0 && !G.total_exact) { int64_t t = 0; if (int rc = d2h_pinned(&t, G.d_off.as<int64_t>() + G.rows, 8, stream)) return rc; G.total = t; G.total_exact = true; }
        off.assign((size_t)G.rows + 1, 0); nbr.assign((size_t)G.total, 0);
        if (int rc = d2h_pinned(off.data(), G.d_off.p, off.size() * 8, stream)) return rc;
        if (G.total > 0) { if (int rc = d2h_pinned(nbr.data(), G.d_nbr.p, nbr.size() * 4, stream)) return rc; }
        return HS_OK;
    }

    // dynamic LDS of the one-wavefront-per-instance kernels: nodes kept in LDS (wider windows use global scratch)
    static int lds_nodes(int max_m, int ints_per_node, int limit_bytes) {
        const int cap = ((std::max(max_m, 1) + 63) / 64) * 64;
        return std::min(cap, (limit_bytes / (ints_per_node * 4)) / 64 * 64);
    }

    std::vector<int64_t>* tap_run_off = nullptr; std::vector<int32_t>* tap_run_labels = nullptr; hs::SrChainRoutes* tap_routes = nullptr;
    void tap_chain(std::vector<int64_t>* run_off, std::vector<int32_t>* run_labels, hs::SrChainRoutes* routes) override { tap_run_off = run_off; tap_run_labels = run_labels; tap_routes = routes; }
    int cw_chain(const hs::CwChain& ch, std::vector<int32_t>& labels, std::vector<int32_t>& final_labels, std::vector<uint8_t>& final_ok,
                 float k_ms[3], hs::SrChainStats* stats) override {
        if (int rc = settle_simdiff()) return rc;   // (a batch without graph windows never built graphs)
        const int Wc = (int)ch.win.size();
        const int64_t n_inst = (int64_t)ch.seed_col.size();
        const int64_t total_m = ch.chain_row0.back();
        if (n_inst > 0x7fffffff) { set_error("Chinese Whispers: too many runs in one call"); return HS_EINVAL; }
        // per-SNP runs: window, slab offset (the runs of a window are contiguous: K * m labels); small windows go to the
        // row-packed kernel, the others to the one-wavefront-per-run kernel
        std::vector<int32_t> inst_win((size_t)n_inst), list_big, list_lanes, unit_win, unit_inst0, unit_n;
        const int lanes_cap = 64;     // windows up to 64 reads: one run per lane (k_cw_seeded_lanes)
        int max_m_small = 1;
        std::vector<int64_t> inst_slab((size_t)n_inst), chain_slab0((size_t)Wc), big_scr, tail_scr((size_t)Wc, 0);
        int64_t slab = 0, big_scr_total = 0, tail_scr_total = 0;
        int max_m_big = 1, max_m_chain = 1;
        bool all_lanes = true;      // every window of the chain narrow enough for one run per lane (the usual case): the lists are filled by the group's threads
        for (int k = 0; k < Wc && all_lanes; ++k) all_lanes = G.win_m[(size_t)ch.win[(size_t)k]] <= lanes_cap;
        if (all_lanes) {
            for (int k = 0; k < Wc; ++k) {
                const int m = G.win_m[(size_t)ch.win[(size_t)k]];
                chain_slab0[(size_t)k] = slab;
                max_m_chain = std::max(max_m_chain, m);
                slab += (ch.win_seed_begin[(size_t)k + 1] - ch.win_seed_begin[(size_t)k]) * (int64_t)m;
            }
            list_lanes.resize((size_t)n_inst);
            hs::hs_parallel_for(Wc, std::min(8, host_threads()), [&](int k) {
                const int w = ch.win[(size_t)k];
                const int m = G.win_m[(size_t)w];
                int64_t sl = chain_slab0[(size_t)k];
                for (int64_t i = ch.win_seed_begin[(size_t)k]; i < ch.win_seed_begin[(size_t)k + 1]; ++i) { inst_win[(size_t)i] = w; inst_slab[(size_t)i] = sl; sl += m; list_lanes[(size_t)i] = (int32_t)i; }
            });
        } else
        for (int k = 0; k < Wc; ++k) {
            const int w = ch.win[(size_t)k];
            const int m = G.win_m[(size_t)w];
            chain_slab0[(size_t)k] = slab;
            max_m_chain = std::max(max_m_chain, m);
            for (int64_t i = ch.win_seed_begin[(size_t)k]; i < ch.win_seed_begin[(size_t)k + 1]; ++i) {
                inst_win[(size_t)i] = w; inst_slab[(size_t)i] = slab; slab += m;
                if (m > HS_CWR_CAP) { list_big.push_back((int32_t)i); max_m_big = std::max(max_m_big, m); }
                else if (m <= lanes_cap) list_lanes.push_back((int32_t)i);
            }
            if (m <= HS_CWR_CAP && m > lanes_cap) {      // units of up to eight runs of this window for the row-packed kernel
                max_m_small = std::max(max_m_small, m);
                for (int64_t i = ch.win_seed_begin[(size_t)k]; i < ch.win_seed_begin[(size_t)k + 1]; i += 8) {
                    unit_win.push_back(w); unit_inst0.push_back((int32_t)i);
                    unit_n.push_back((int32_t)std::min<int64_t>(8, ch.win_seed_begin[(size_t)k + 1] - i));
                }
            }
        }
        const int cap_big = lds_nodes(max_m_big, 2, 96 * 1024);
        for (int32_t i : list_big) {
            const int m = G.win_m[(size_t)inst_win[(size_t)i]];
            big_scr.push_back(big_scr_total);
            if (m > cap_big) big_scr_total += 2 * (int64_t)m;
        }
        const int cap_tail = lds_nodes(max_m_chain, 7, 56 * 1024);
        if (tap_routes) {      // (test taps: the sizes of the lists above)
            hs::SrChainRoutes& rt = *tap_routes;
            rt = hs::SrChainRoutes();
            rt.all_lanes = all_lanes ? 1 : 0; rt.runs_lanes = (int64_t)list_lanes.size(); rt.units_rows = (int64_t)unit_win.size();
            for (int32_t n : unit_n) rt.runs_rows += n;
            rt.runs_wave = (int64_t)list_big.size();
            for (int32_t i : list_big) if (G.win_m[(size_t)inst_win[(size_t)i]] > cap_big) rt.runs_wave_scratch++;
            rt.cap_tail = cap_tail;
            for (int k = 0; k < Wc; ++k) { const int m = G.win_m[(size_t)ch.win[(size_t)k]]; if (m <= 64) rt.tail_narrow++; else if (m > cap_tail) rt.tail_scratch++; else rt.tail_lds++; }
        }
        // two launches of the tail: the windows of at most 64 nodes with LDS for 64 (more wavefronts per CU), then the wider ones
        std::vector<int32_t> tail_list((size_t)Wc);
        int n_tail_small = 0;
        {
            int wide = 0;
            for (int k = 0; k < Wc; ++k) if (G.win_m[(size_t)ch.win[(size_t)k]] <= 64) n_tail_small++;
            int at_small = 0;
            for (int k = 0; k < Wc; ++k) { if (G.win_m[(size_t)ch.win[(size_t)k]] <= 64) tail_list[(size_t)at_small++] = k; else tail_list[(size_t)(n_tail_small + wide++)] = k; }
        }
        for (int k = 0; k < Wc; ++k) {
            const int m = G.win_m[(size_t)ch.win[(size_t)k]];
            tail_scr[(size_t)k] = tail_scr_total;
            if (m > cap_tail) tail_scr_total += 7 * (int64_t)m + (m & 1);      // keeps the next window's doubles 8-byte aligned
        }
        DBuf d_ll, d_sets, d_names, d_slots, d_alive, d_ovf, d_ovf_n, d_iw, d_is, d_seed, d_uw, d_ui, d_un, d_lb, d_bs, d_cw, d_cr0, d_csb, d_cs0, d_ts, d_slab, d_gs, d_l3, d_final, d_ok, d_stat,
            d_cpos, d_sf, d_sl, d_plo, d_phi, d_tl;
        if (resident_cols != &ch && !adopted) {   // normally uploaded by simdiff_columns already
            col_pack.add(ch.col_off, d_col_off); col_pack.add(ch.col_idx, d_col_idx); col_pack.add(ch.col_code, d_col_code);
            if (int rc = col_pack.commit(stream)) return rc;
            resident_cols = &ch;
        }
        const bool finish = ch.finish_on_device && !std::getenv("HS_FINISH_ON_HOST");
        UploadPack pk;
        pk.add(inst_win, d_iw); pk.add(inst_slab, d_is); pk.add(ch.seed_col, d_seed); pk.add(unit_win, d_uw); pk.add(unit_inst0, d_ui); pk.add(unit_n, d_un); pk.add(list_big, d_lb); pk.add(list_lanes, d_ll);
        pk.add(big_scr, d_bs); pk.add(ch.win, d_cw); pk.add(ch.chain_row0, d_cr0); pk.add(ch.win_seed_begin, d_csb); pk.add(chain_slab0, d_cs0);
        pk.add(tail_scr, d_ts); pk.add(tail_list, d_tl);
        if (finish) { pk.add(ch.col_pos, d_cpos); pk.add(ch.win_snp_first, d_sf); pk.add(ch.win_snp_last, d_sl); pk.add(ch.win_pos_lo, d_plo); pk.add(ch.win_pos_hi, d_phi); }
        if (int rc = pk.commit(stream)) return rc;
        if (int rc = d_slab.alloc(std::max<size_t>((size_t)slab, 1) * 4)) return rc;
        if (int rc = d_gs.alloc(std::max<size_t>((size_t)std::max(big_scr_total, tail_scr_total), 2) * 4)) return rc;
        if (int rc = d_l3.alloc(std::max<size_t>((size_t)total_m, 1) * 4)) return rc;
        if (int rc = d_final.alloc(std::max<size_t>((size_t)total_m, 1) * 4)) return rc;
        if (int rc = d_ok.alloc(std::max<size_t>((size_t)Wc, 1))) return rc;
        if (int rc = d_stat.alloc(416)) return rc;    // {sweeps, bytes} of the per-SNP runs, {sweeps, bytes} of the window tails, histogram of sweeps per run [16]
        hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, d_stat.as<uint4>(), 26ll, 0u);
        EventPair e1, e2;
        if (int rc = e1.init()) return rc;
        if (int rc = e2.init()) return rc;
        // ---- per-SNP runs, seeded on the device from the SNP columns ----
        HS_HIP(ev_rec(e1.a, stream));
        if (!list_lanes.empty()) {
            const int n = (int)list_lanes.size();
            const size_t npad = ((size_t)n + 63) & ~(size_t)63;
            if (int rc = d_sets.alloc(npad * 128)) return rc;
            if (int rc = d_names.alloc(npad * 16)) return rc;
            if (int rc = d_slots.alloc(npad * 64)) return rc;
            if (int rc = d_alive.alloc(npad)) return rc;
            if (int rc = d_ovf.alloc((size_t)n * 4)) return rc;
            if (int rc = d_ovf_n.alloc(16)) return rc;
            hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, d_ovf_n.as<uint4>(), 1ll, 0u);
            if (int rc = kc.begin(HS_K_CW_SEED_SETS, stream)) return rc;
            hipLaunchKernelGGL(hsdev::k_cw_seed_sets, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, G.d_row0.as<int64_t>(), G.d_ids.as<int32_t>(), d_ll.as<int32_t>(), n,
                               d_iw.as<int32_t>(), d_seed.as<int64_t>(), d_col_off.as<int64_t>(), d_col_idx.as<int32_t>(), d_col_code.as<uint8_t>(),
                               d_sets.as<unsigned long long>(), d_names.as<uint8_t>(), d_slots.as<uint8_t>(), d_alive.as<uint8_t>(), d_ovf.as<int32_t>(), d_ovf_n.as<int32_t>());
            HS_HIP(hipGetLastError());
            if (int rc = kc.end((int64_t)npad * 209 + 5 * (int64_t)n * 40, stream)) return rc;      // sets, names, slots, alive out per run; the seeding column (about 40 entries) in
            if (int rc = kc.begin(HS_K_CW_SEEDED, stream)) return rc;
            hipLaunchKernelGGL(hsdev::k_cw_seeded_lanes, dim3((unsigned)(npad / 64)), dim3(64), 0, stream, G.d_off.as<int64_t>(), G.d_row0.as<int64_t>(), G.d_visit_n.as<int32_t>(),
                               G.d_prog_info.as<uint32_t>(), G.d_prog_adj.as<unsigned long long>(), d_ll.as<int32_t>(), n, d_iw.as<int32_t>(), d_is.as<int64_t>(),
                               d_sets.as<unsigned long long>(), d_names.as<uint8_t>(), d_slots.as<uint8_t>(), d_alive.as<uint8_t>(), d_slab.as<int32_t>(), d_stat.as<unsigned long long>());
            HS_HIP(hipGetLastError());
            if (int rc = kc.end((int64_t)npad * 209, stream)) return rc;      // + sweeps * (4 nnz + 8 m) per run, counted by the kernel itself (added below)
            const bool timing = std::getenv("HS_TIMING") != nullptr;
            if (timing || tap_routes) {
                int32_t n_ovf = 0;
                if (int rc = d2h_pinned(&n_ovf, d_ovf_n.p, 4, stream)) return rc;
                if (tap_routes) tap_routes->runs_overflow = n_ovf;
                if (timing) {
                    std::fprintf(stderr, "[hs timing] sr: %d per-SNP runs one per lane, %d of them with more than 16 labels alive (-> one wavefront each); %zu runs in units of 8, %zu one wavefront each\n",
                                 n, n_ovf, unit_win.size() * 8, list_big.size());
                }
            }
            // the few runs with more labels alive than slots: one wavefront each, the list and its length are on the device
            if (int rc = kc.begin(HS_K_CW_SEEDED_WIDE, stream)) return rc;
            hipLaunchKernelGGL(hsdev::k_cw_seeded_wave, dim3((unsigned)std::min(n, 1024)), dim3(64), (size_t)64 * 8, stream, G.d_off.as<int64_t>(), G.d_nbr.as<int32_t>(),
                               G.d_row0.as<int64_t>(), G.d_ids.as<int32_t>(), G.d_visit.as<int32_t>(), G.d_visit_n.as<int32_t>(), d_ovf.as<int32_t>(), 0, d_ovf_n.as<int32_t>(),
                               d_iw.as<int32_t>(), d_seed.as<int64_t>(), d_is.as<int64_t>(), d_col_off.as<int64_t>(), d_col_idx.as<int32_t>(),
                               d_col_code.as<uint8_t>(), 64, (int32_t*)nullptr, (const int64_t*)nullptr, d_slab.as<int32_t>(), d_stat.as<unsigned long long>());
            HS_HIP(hipGetLastError());
            if (int rc = kc.end(0, stream)) return rc;
        }
        if (!unit_win.empty() || !list_big.empty()) { if (int rc = kc.begin(HS_K_CW_SEEDED_WIDE, stream)) return rc; }
        if (!unit_win.empty()) {
            const int n = (int)unit_win.size();
            const int m_cap = std::max(16, (max_m_small + 15) & ~15);
            const int cnt_cap = std::max(m_cap, 256);
            const int prog_cap = std::max(2048, m_cap * 32);
            const size_t lds = (size_t)2 * m_cap * 4 + (size_t)8 * cnt_cap * 4 + (size_t)prog_cap + (size_t)8 * m_cap;
            if (lds > 48 * 1024)
                HS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hsdev::k_cw_seeded_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(hsdev::k_cw_seeded_rows, dim3((unsigned)n), dim3(128), lds, stream, G.d_off.as<int64_t>(), G.d_nbr.as<int32_t>(),
                               G.d_row0.as<int64_t>(), G.d_ids.as<int32_t>(), G.d_visit.as<int32_t>(), G.d_visit_n.as<int32_t>(), G.d_prog_info.as<uint32_t>(),
                               G.d_prog_bytes.as<uint8_t>(), G.d_prog_steps.as<int32_t>(), d_uw.as<int32_t>(), d_ui.as<int32_t>(), d_un.as<int32_t>(), n, d_seed.as<int64_t>(), d_is.as<int64_t>(), d_col_off.as<int64_t>(), d_col_idx.as<int32_t>(),
                               d_col_code.as<uint8_t>(), m_cap, prog_cap, d_slab.as<int32_t>(), d_stat.as<unsigned long long>());
            HS_HIP(hipGetLastError());
        }
        if (!list_big.empty()) {
            const int n = (int)list_big.size();
            const size_t lds = (size_t)cap_big * 8;
            if (lds > 48 * 1024)
                HS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hsdev::k_cw_seeded_wave), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(hsdev::k_cw_seeded_wave, dim3((unsigned)n), dim3(64), lds, stream, G.d_off.as<int64_t>(), G.d_nbr.as<int32_t>(),
                               G.d_row0.as<int64_t>(), G.d_ids.as<int32_t>(), G.d_visit.as<int32_t>(), G.d_visit_n.as<int32_t>(), d_lb.as<int32_t>(), n, (const int32_t*)nullptr,
                               d_iw.as<int32_t>(), d_seed.as<int64_t>(), d_is.as<int64_t>(), d_col_off.as<int64_t>(), d_col_idx.as<int32_t>(),
                               d_col_code.as<uint8_t>(), cap_big, d_gs.as<int32_t>(), d_bs.as<int64_t>(), d_slab.as<int32_t>(), d_stat.as<unsigned long long>());
            HS_HIP(hipGetLastError());
        }
        if (!unit_win.empty() || !list_big.empty()) { if (int rc = kc.end(0, stream)) return rc; }
        HS_HIP(ev_rec(e1.b, stream));
        // ---- the rest of the window's chain, labels in LDS from here to the finished clusters ----
        HS_HIP(ev_rec(e2.a, stream));
        if (int rc = kc.begin(HS_K_WINDOW_TAIL, stream)) return rc;
        if (Wc > 0) {
            const size_t lds = (size_t)cap_tail * 7 * 4 + HS_TAIL_MAP_EXTRA;
            if (lds > 32 * 1024)
                HS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hsdev::k_window_tail), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            for (int part = 0; part < 2; ++part) {
                const int n_part = part == 0 ? n_tail_small : Wc - n_tail_small;
                if (n_part == 0) continue;
                const int cap = part == 0 ? std::min(cap_tail, 64) : cap_tail;
                hipLaunchKernelGGL(hsdev::k_window_tail, dim3((unsigned)n_part), dim3(64), (size_t)cap * 7 * 4 + HS_TAIL_MAP_EXTRA, stream, G.d_off.as<int64_t>(), G.d_nbr.as<int32_t>(), G.d_row0.as<int64_t>(),
                                   G.d_ids.as<int32_t>(), G.d_visit.as<int32_t>(), G.d_visit_n.as<int32_t>(), G.d_fe.as<uint8_t>(), G.d_prog_info.as<uint32_t>(),
                                   G.d_prog_adj.as<unsigned long long>(), d_cw.as<int32_t>(), d_cr0.as<int64_t>(),
                                   d_csb.as<int64_t>(), d_cs0.as<int64_t>(), d_slab.as<int32_t>(), d_tl.as<int32_t>() + (part == 0 ? 0 : n_tail_small), n_part, d_col_off.as<int64_t>(),
                                   d_col_idx.as<int32_t>(), d_col_code.as<uint8_t>(), d_cpos.as<int32_t>(), d_sf.as<int64_t>(), d_sl.as<int64_t>(), d_plo.as<int32_t>(), d_phi.as<int32_t>(),
                                   finish ? 1 : 0, cap, d_gs.as<int32_t>(), d_ts.as<int64_t>(), d_l3.as<int32_t>(), d_final.as<int32_t>(), d_ok.as<uint8_t>(),
                                   d_stat.as<unsigned long long>() + 2);
            }
            HS_HIP(hipGetLastError());
        }
        if (int rc = kc.end(4 * slab + 8 * total_m, stream)) return rc;   // the runs' labels in, the two label arrays out (+ its two runs, below)
        HS_HIP(ev_rec(e2.b, stream));
        {
            // the finished labels and the per-window verdict come back in one shipment with the counters (and the size of the graphs, which
            // the host has not asked for until now); the labels of the third run are only fetched when some window has to be finished by the
            // host code (few or none)
            HBuf h, h4;
            const size_t o_nnz = 416, o_final = 512, o_ok = o_final + (((size_t)total_m * 4 + 255) & ~(size_t)255);
            if (int rc = h4.alloc(o_ok + (size_t)Wc + 256)) return rc;
            Shipment sh;
            sh.add(h4.p, d_stat.p, 416);
            const int64_t* h_nnz = sh.add_word((char*)h4.p + o_nnz, G.d_off.as<int64_t>() + G.rows);      // (d_off[rows]; the block is 16-byte aligned)
            bool need_chain_labels = !finish || tap_run_labels != nullptr;
            if (finish) {
                sh.add((char*)h4.p + o_final, d_final.p, (size_t)total_m * sizeof(int32_t));
                sh.add((char*)h4.p + o_ok, d_ok.p, (size_t)Wc);
            }
            if (int rc = kc.begin(HS_K_SHIP, stream)) return rc;
            if (int rc = sh.launch(stream, 64)) return rc;
            if (int rc = kc.end(0, stream)) return rc;
            if (int rc = stream_wait(stream)) return rc;
            if (finish) {
                final_labels.resize((size_t)total_m); final_ok.resize((size_t)Wc);
                std::memcpy(final_labels.data(), (const char*)h4.p + o_final, (size_t)total_m * sizeof(int32_t));
                std::memcpy(final_ok.data(), (const char*)h4.p + o_ok, (size_t)Wc);
                for (uint8_t ok : final_ok) if (!ok) { need_chain_labels = true; break; }
            }
            if (need_chain_labels) {
                labels.resize((size_t)total_m);
                if (int rc = h.alloc(std::max<size_t>((size_t)total_m, 1) * sizeof(int32_t))) return rc;
                if (int rc = copy_d2h(h.p, d_l3.p, (size_t)total_m * sizeof(int32_t), stream)) return rc;
                std::memcpy(labels.data(), h.p, (size_t)total_m * sizeof(int32_t));
            } else labels.clear();
            if (tap_run_labels && tap_run_off) {      // (test taps: the per-SNP runs' labels as the kernels left them)
                tap_run_labels->resize((size_t)slab);
                if (slab) { if (int rc = d2h_pinned(tap_run_labels->data(), d_slab.p, (size_t)slab * sizeof(int32_t), stream)) return rc; }
                tap_run_off->assign(inst_slab.begin(), inst_slab.end()); tap_run_off->push_back(slab);
            }
            if (!G.total_exact) { G.total = *h_nnz; G.total_exact = true; }
            if (int rc = graph_rows_settle(G, &kc)) return rc;
            const unsigned long long* st = (const unsigned long long*)h4.p;
            if (stats) { stats->n_instances = n_inst + 2 * (int64_t)Wc; stats->sweeps = (int64_t)(st[0] + st[2]); stats->bytes = (int64_t)(st[1] + st[3]); stats->graph_nnz = G.total; }
            if (std::getenv("HS_TIMING")) {
                std::string h;
                for (int k = 0; k < 16; ++k) h += " " + std::to_string((unsigned long long)st[4 + k]);
                std::fprintf(stderr, "[hs timing] sr: per-SNP Chinese-Whispers runs by number of sweeps (0..15+):%s\n", h.c_str());
#ifdef HS_TAIL_DIAG      // (build with -DHS_TAIL_DIAG: shader cycles of the sections of k_window_tail, summed over the windows)
                std::fprintf(stderr, "[hs timing] sr: k_window_tail cycles: merged ids %llu, two runs + small clusters %llu, renumbering %llu, merge_close_clusters %llu, merge_wrongly_split_haplotypes: slots + map %llu, SNPs %llu, link counts %llu, links + output %llu; SNPs fast %llu slow %llu, keys %llu, windows with map %llu, clusters %llu\n",
                             (unsigned long long)st[20], (unsigned long long)st[21], (unsigned long long)st[22], (unsigned long long)st[23], (unsigned long long)st[25], (unsigned long long)st[26],
                             (unsigned long long)st[27], (unsigned long long)st[24], (unsigned long long)st[28], (unsigned long long)st[29], (unsigned long long)st[30], (unsigned long long)st[31], (unsigned long long)st[32]);
#endif
#ifdef HS_CW_DIAG
                h.clear(); for (int k = 0; k < 16; ++k) h += " " + std::to_string((unsigned long long)st[20 + k]);
                std::fprintf(stderr, "[hs timing] sr: runs by labels alive after seeding (0..15+):%s\n", h.c_str());
                h.clear(); for (int k = 0; k < 16; ++k) h += " " + std::to_string((unsigned long long)st[36 + k]);
                std::fprintf(stderr, "[hs timing] sr: runs by m/16:%s\n", h.c_str());
#endif
            }
            KernelClock::add_bytes(HS_K_CW_SEEDED, (int64_t)st[1]);
            KernelClock::add_bytes(HS_K_WINDOW_TAIL, (int64_t)st[3]);
            kc.flush();
        }
        float m = 0;
        if (int rc = e1.ms(&m)) return rc; k_ms[0] += m;
        if (int rc = e2.ms(&m)) return rc; k_ms[1] += m;
        return HS_OK;
    }
    int cw(hs::CwWave& wv, float* k_ms) override {
        const int n_inst = (int)wv.inst_win.size();
        if (n_inst == 0) return HS_OK;
        int max_m = 1;
        for (int w : wv.inst_win) max_m = std::max(max_m, G.win_m[(size_t)w]);
        const int cap = lds_nodes(max_m, 2, 96 * 1024);
        std::vector<int64_t> scr((size_t)n_inst, 0);
        int64_t scr_total = 0;
        for (int k = 0; k < n_inst; ++k) { const int m = G.win_m[(size_t)wv.inst_win[(size_t)k]]; scr[(size_t)k] = scr_total; if (m > cap) scr_total += 2 * (int64_t)m; }
        DBuf d_iw, d_lo, d_lab, d_scr, d_gs;
        UploadPack pk;
        pk.add(wv.inst_win, d_iw); pk.add(wv.inst_label_off, d_lo); pk.add(wv.labels, d_lab); pk.add(scr, d_scr);
        if (int rc = pk.commit(stream)) return rc;
        if (int rc = d_gs.alloc(std::max<size_t>((size_t)scr_total, 2) * 4)) return rc;
        EventPair ev; if (int rc = ev.init()) return rc;
        HS_HIP(ev_rec(ev.a, stream));
        if (int rc = kc.begin(HS_K_CW_LOCAL, stream)) return rc;
        const size_t lds = (size_t)cap * 8;
        if (lds > 48 * 1024)
            HS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hsdev::k_cw_local), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(hsdev::k_cw_local, dim3((unsigned)n_inst), dim3(64), lds, stream, G.d_off.as<int64_t>(), G.d_nbr.as<int32_t>(), G.d_row0.as<int64_t>(),
                           G.d_visit.as<int32_t>(), G.d_visit_n.as<int32_t>(), G.d_fe.as<uint8_t>(), d_iw.as<int32_t>(), d_lo.as<int64_t>(), n_inst, cap,
                           d_gs.as<int32_t>(), d_scr.as<int64_t>(), d_lab.as<int32_t>());
        HS_HIP(hipGetLastError());
        if (int rc = kc.end(8 * (int64_t)wv.labels.size(), stream)) return rc;
        HS_HIP(ev_rec(ev.b, stream));
        if (int rc = d2h_pinned(wv.labels.data(), d_lab.p, wv.labels.size() * sizeof(int32_t), stream)) return rc;
        float m = 0; if (int rc = ev.ms(&m)) return rc;
        if (k_ms) *k_ms += m;
        return HS_OK;
    }
};

}  // namespace

