// hs_capi_multi.inc -- part of hs_capi.hip: several GPUs in one process (hs_devices, hs_sr_run, hs_cv_run_host: contigs sharded over the
// visible devices by longest-processing-time, one host thread and device per shard, results merged in contig order).
// ---------------------------------------------------------------------------------------------------
// Several GPUs in one process: contigs are independent in both stages (call_variants.cpp:1276-1280, separate_reads.cpp:
// 1506-1508), so the stage-level calls shard them over the devices of hs_devices() -- longest-processing-time on a weight
// per contig -- one host thread (with its worker pool and HIP stream) per device; the per-shard results come back over each
// device's own PCIe link and are merged in contig order. HS_DEVICES="0,1,.." picks the devices (default: every visible
// one); a device may be listed more than once (two shards on one GPU: how the path is exercised on a single-GPU box).
// ---------------------------------------------------------------------------------------------------
static std::vector<int> device_list() {   // (extern "C" linkage block: plain static function)
    std::vector<int> d;
    if (const char* e = std::getenv("HS_DEVICES")) {
        for (const char* p = e; *p;) { char* end = nullptr; const long v = std::strtol(p, &end, 10); if (end == p) break; d.push_back((int)v); p = *end == ',' ? end + 1 : end; }
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    if (d.empty()) for (int i = 0; i < n; ++i) d.push_back(i);
    for (int& v : d) if (v < 0 || v >= n) v = 0;
    return d;
}
int hs_devices(int32_t* out, int32_t cap) {
    const std::vector<int> d = device_list();
    for (size_t i = 0; i < d.size() && (int32_t)i < cap; ++i) out[i] = d[i];
    return (int)d.size();
}
// longest-processing-time assignment, deterministic (ties by index); shards hold ascending contig ids
static std::vector<std::vector<int>> lpt_shards(const std::vector<double>& w, int parts) {
    std::vector<int> order(w.size());
    for (size_t i = 0; i < w.size(); ++i) order[i] = (int)i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return w[(size_t)a] != w[(size_t)b] ? w[(size_t)a] > w[(size_t)b] : a < b; });
    std::vector<double> load((size_t)parts, 0.0);
    std::vector<std::vector<int>> sh((size_t)parts);
    for (int i : order) {
        int best = 0;
        for (int k = 1; k < parts; ++k) if (load[(size_t)k] < load[(size_t)best]) best = k;
        sh[(size_t)best].push_back(i); load[(size_t)best] += w[(size_t)i];
    }
    for (auto& v : sh) std::sort(v.begin(), v.end());
    return sh;
}
// f(shard) on one host thread per shard, each bound to its device; first failure wins
static int run_on_devices(const std::vector<int>& devs, const std::function<int(int)>& f) {
    const int D = (int)devs.size();
    std::vector<int> rcs((size_t)D, 0);
    std::vector<std::string> errs((size_t)D);
    std::vector<std::thread> th;
    for (int k = 0; k < D; ++k)
        th.emplace_back([&, k] {
            if (hipSetDevice(devs[(size_t)k]) != hipSuccess) { rcs[(size_t)k] = HS_EHIP; errs[(size_t)k] = "hipSetDevice failed"; return; }
            set_wait_policy();
            rcs[(size_t)k] = f(k);
            if (rcs[(size_t)k]) errs[(size_t)k] = hs_last_error();
        });
    for (auto& t : th) t.join();
    for (int k = 0; k < D; ++k) if (rcs[(size_t)k]) { set_error(errs[(size_t)k]); return rcs[(size_t)k]; }
    return HS_OK;
}

// ---- test taps of the clustering chain (include/hairsplitter_hip.h: hs_sr_taps) ----
void hs_sr_taps_destroy(hs_sr_taps* t) {
    if (!t) return;
    std::free(t->win_contig); std::free(t->win_start); std::free(t->win_row0); std::free(t->mask_ids); std::free(t->run_begin); std::free(t->run_snp); std::free(t->run_off);
    std::free(t->run_labels); std::free(t->third);
    std::free(t->g_win_contig); std::free(t->g_win_kind); std::free(t->g_win_row0); std::free(t->g_mask_ids); std::free(t->g_nbr_off); std::free(t->g_nbr);
    std::free(t->g_plane_n); std::free(t->g_words); std::free(t->g_plane_off); std::free(t->g_alt); std::free(t->g_ref); std::free(t->g_n_reads); std::free(t->g_out_off);
    std::free(t->g_read_base); std::free(t->g_pos_orig); std::free(t->g_matrix);
    std::free(t);
}
int hs_sr_run_taps(const hs_sr_contig* contigs, int32_t n_contigs, int32_t window_size, float error_rate, int32_t low_memory, uint32_t seed,
                   int32_t n_threads, int32_t mode, hs_sr_result** out, hs_sr_taps** taps) {
    if (int rc = require_device()) return rc;
    if (!out || !taps || n_contigs < 0 || (mode != HS_SR_TAPS_CHAIN && mode != HS_SR_TAPS_GRAPHS)) { set_error("hs_sr_run_taps: bad arguments"); return HS_EINVAL; }
    hs::SrTaps tp;
    tp.graphs = mode == HS_SR_TAPS_GRAPHS;
    {
        HipSrOps ops;
        if (int rc = hs::sr_run(ops, contigs, n_contigs, window_size, error_rate, low_memory, seed, n_threads, out, nullptr, nullptr, &tp)) return rc;
    }
    // the runs' labels are window-local node ids: as read indices here (node j of a window is its j-th read)
    const size_t Wc = tp.win_contig.size();
    for (size_t k = 0; k < Wc; ++k) {
        const int64_t r0 = tp.win_row0[k], m = tp.win_row0[k + 1] - r0;
        for (int64_t i = tp.run_begin[k]; i < tp.run_begin[k + 1]; ++i)
            for (int64_t j = 0; j < m; ++j) { int32_t& l = tp.run_labels[(size_t)(tp.run_off[(size_t)i] + j)]; if (l >= 0 && l < m) l = tp.mask_ids[(size_t)(r0 + l)]; }
    }
    auto dup_vec = [](const auto& v) { using T = typename std::decay<decltype(v)>::type::value_type; T* p = (T*)std::malloc(std::max<size_t>(1, v.size()) * sizeof(T)); if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T)); return p; };
    hs_sr_taps* t = (hs_sr_taps*)std::calloc(1, sizeof(hs_sr_taps));
    t->n_windows = (int32_t)Wc;
    t->win_contig = dup_vec(tp.win_contig); t->win_start = dup_vec(tp.win_start); t->win_row0 = dup_vec(tp.win_row0); t->mask_ids = dup_vec(tp.mask_ids);
    t->run_begin = dup_vec(tp.run_begin); t->run_snp = dup_vec(tp.run_snp); t->run_off = dup_vec(tp.run_off); t->run_labels = dup_vec(tp.run_labels); t->third = dup_vec(tp.third);
    {
        const hs::SrChainRoutes& rt = tp.routes;
        t->all_lanes = rt.all_lanes; t->cap_tail = rt.cap_tail; t->runs_lanes = rt.runs_lanes; t->runs_overflow = rt.runs_overflow; t->runs_rows = rt.runs_rows;
        t->units_rows = rt.units_rows; t->runs_wave = rt.runs_wave; t->runs_wave_scratch = rt.runs_wave_scratch; t->tail_narrow = rt.tail_narrow;
        t->tail_lds = rt.tail_lds; t->tail_scratch = rt.tail_scratch;
    }
    if (tp.graphs) {
        const hs::SrGraphTaps& f = tp.front;
        t->g_n_windows = (int32_t)f.win_contig.size();
        t->g_win_contig = dup_vec(f.win_contig); t->g_win_kind = dup_vec(f.win_kind); t->g_win_row0 = dup_vec(f.win_row0); t->g_mask_ids = dup_vec(f.mask_ids);
        t->g_nbr_off = dup_vec(f.nbr_off); t->g_nbr = dup_vec(f.nbr);
        t->g_n_contigs = (int32_t)f.plane_n.size();
        t->g_plane_n = dup_vec(f.plane_n); t->g_words = dup_vec(f.words); t->g_plane_off = dup_vec(f.plane_off); t->g_alt = dup_vec(f.alt); t->g_ref = dup_vec(f.ref);
        t->g_n_reads = dup_vec(f.n_reads); t->g_out_off = dup_vec(f.out_off); t->g_read_base = dup_vec(f.read_base); t->g_pos_orig = dup_vec(f.pos_orig);
        t->g_n_pos_orig = (int64_t)f.pos_orig.size(); t->g_n_plane_words = (int64_t)f.alt.size(); t->g_n_pairs = (int64_t)f.matrix.size() / 2;
        t->g_matrix = dup_vec(f.matrix);
        t->g_rows_on_host = f.rows_on_host; t->g_rows_late = f.rows_late; t->g_row_waves = f.row_waves;
    }
    *taps = t;
    return HS_OK;
}

int hs_sr_run(const hs_sr_contig* contigs, int32_t n_contigs, int32_t window_size, float error_rate, int32_t low_memory,
              uint32_t seed, int32_t n_threads, hs_sr_result** out) {
    if (int rc = require_device()) return rc;
    if (!out || n_contigs < 0) { set_error("hs_sr_run: bad arguments"); return HS_EINVAL; }
    const std::vector<int> devs = device_list();
    if (devs.size() <= 1 || n_contigs < 2) {
        HipSrOps ops;
        return hs::sr_run(ops, contigs, n_contigs, window_size, error_rate, low_memory, seed, n_threads, out);
    }
    // weight of a contig in stage 4: its sim / diff matrices (N^2) and its windows (~ length x depth)
    std::vector<double> w((size_t)n_contigs);
    for (int c = 0; c < n_contigs; ++c) w[(size_t)c] = 16.0 * contigs[c].n_reads * (double)contigs[c].n_reads + (double)contigs[c].n_snps * contigs[c].n_reads + 1.0;
    const int D = (int)std::min<size_t>(devs.size(), (size_t)n_contigs);
    const std::vector<std::vector<int>> shards = lpt_shards(w, D);
    std::vector<hs_sr_result*> parts((size_t)D, nullptr);
    const int per = n_threads > 0 ? std::max(1, n_threads / D) : 0;
    const int rc = run_on_devices(std::vector<int>(devs.begin(), devs.begin() + D), [&](int k) {
        std::vector<hs_sr_contig> sub;
        for (int c : shards[(size_t)k]) sub.push_back(contigs[c]);
        HipSrOps ops;
        return hs::sr_run(ops, sub.data(), (int32_t)sub.size(), window_size, error_rate, low_memory, seed, per, &parts[(size_t)k]);
    });
    if (rc) { for (hs_sr_result* r : parts) if (r) hs::free_sr_result(r); return rc; }
    // merge in contig order
    std::vector<std::pair<int, int>> where((size_t)n_contigs);   // contig -> (shard, index in shard)
    for (int k = 0; k < D; ++k) for (size_t i = 0; i < shards[(size_t)k].size(); ++i) where[(size_t)shards[(size_t)k][i]] = std::make_pair(k, (int)i);
    hs_sr_result* R = (hs_sr_result*)std::calloc(1, sizeof(hs_sr_result));
    int64_t W = 0, NL = 0;
    for (hs_sr_result* r : parts) { W += r->win_off[r->n_contigs]; NL += r->label_off[r->win_off[r->n_contigs]]; }
    R->n_contigs = n_contigs;
    R->win_off = (int64_t*)std::malloc(((size_t)n_contigs + 1) * sizeof(int64_t));
    R->win_start = (int32_t*)std::malloc((size_t)std::max<int64_t>(1, W) * sizeof(int32_t));
    R->win_end = (int32_t*)std::malloc((size_t)std::max<int64_t>(1, W) * sizeof(int32_t));
    R->label_off = (int64_t*)std::malloc(((size_t)W + 1) * sizeof(int64_t));
    R->labels = hs::sr_labels_alloc((size_t)NL);
    // contig order: where every contig's windows and labels go (prefix sums over the contigs), then the copies on all host threads
    R->win_off[0] = 0; R->label_off[0] = 0;
    std::vector<int64_t> lab0((size_t)n_contigs + 1, 0);
    for (int c = 0; c < n_contigs; ++c) {
        const hs_sr_result* r = parts[(size_t)where[(size_t)c].first];
        const int i = where[(size_t)c].second;
        R->win_off[c + 1] = R->win_off[c] + (r->win_off[i + 1] - r->win_off[i]);
        lab0[(size_t)c + 1] = lab0[(size_t)c] + (r->label_off[r->win_off[i + 1]] - r->label_off[r->win_off[i]]);
    }
    R->label_off[W] = NL;
    hs::hs_parallel_for(n_contigs, host_threads(), [&](int c) {
        const hs_sr_result* r = parts[(size_t)where[(size_t)c].first];
        const int i = where[(size_t)c].second;
        const int64_t q0 = r->win_off[i], nq = r->win_off[i + 1] - q0, w0 = R->win_off[c];
        if (nq == 0) return;
        std::memcpy(R->win_start + w0, r->win_start + q0, (size_t)nq * sizeof(int32_t));
        std::memcpy(R->win_end + w0, r->win_end + q0, (size_t)nq * sizeof(int32_t));
        const int64_t shift = lab0[(size_t)c] - r->label_off[q0];
        for (int64_t q = 0; q < nq; ++q) R->label_off[w0 + q] = r->label_off[q0 + q] + shift;
        std::memcpy(R->labels + lab0[(size_t)c], r->labels + r->label_off[q0], (size_t)(r->label_off[q0 + nq] - r->label_off[q0]) * sizeof(int32_t));
    });
    for (hs_sr_result* r : parts) {
        R->t_device_ms += r->t_device_ms; R->t_host_ms += r->t_host_ms; R->n_cw_instances += r->n_cw_instances;
        for (int k = 0; k < 4; ++k) R->t_kernel_ms[k] += r->t_kernel_ms[k];
        R->t_kernel_graph_ms += r->t_kernel_graph_ms; R->n_graph_rows_host += r->n_graph_rows_host; R->n_windows_finished_on_host += r->n_windows_finished_on_host;
        R->n_cw_sweeps += r->n_cw_sweeps; R->cw_bytes += r->cw_bytes; R->graph_nnz += r->graph_nnz; R->n_graph_rows += r->n_graph_rows; R->simdiff_bytes += r->simdiff_bytes;
        hs::free_sr_result(r);
    }
    *out = R;
    return HS_OK;
}

// Stage 3 from host buffers (what parse_reads / parse_assembly / parse_SAM produce, flattened as for hs_cv_batch_create),
// sharded over hs_devices(): every shard uploads its contigs, the reads its records refer to and their CIGARs to its device,
// runs hs_cv_run there and the results are merged in contig order (error rate over the whole job, call_variants.cpp:1312-1315).
int hs_cv_run_host(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off,
                   int32_t n_reads, const int32_t* h_rec_read, const int32_t* h_rec_pos, const uint8_t* h_rec_strand, const int64_t* h_rec_cig_off,
                   const uint32_t* h_cigar, const int32_t* h_contig_rec_off, float automatic_snp_threshold, int32_t n_threads, hs_cv_result** out) {
    if (int rc = require_device()) return rc;
    if (!out || n_contigs < 0) { set_error("hs_cv_run_host: bad arguments"); return HS_EINVAL; }
    const std::vector<int> devs = device_list();
    if (devs.size() <= 1 || n_contigs < 2) {
        hs_cv_batch* b = nullptr;
        if (int rc = hs_cv_batch_create(h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, h_rec_read, h_rec_pos, h_rec_strand,
                                        h_rec_cig_off, h_cigar, h_contig_rec_off, &b)) return rc;
        const int rc = hs_cv_run(b, automatic_snp_threshold, n_threads, out);
        hs_cv_batch_destroy(b);
        return rc;
    }
    // weight of a contig in stage 3 ~ its aligned bp ~ the bases of the reads aligned to it
    std::vector<double> w((size_t)n_contigs, 1.0);
    for (int c = 0; c < n_contigs; ++c)
        for (int r = h_contig_rec_off[c]; r < h_contig_rec_off[c + 1]; ++r) w[(size_t)c] += (double)(h_read_off[h_rec_read[r] + 1] - h_read_off[h_rec_read[r]]);
    const int D = (int)std::min<size_t>(devs.size(), (size_t)n_contigs);
    const std::vector<std::vector<int>> shards = lpt_shards(w, D);
    std::vector<hs_cv_result*> parts((size_t)D, nullptr);
    const int per = n_threads > 0 ? std::max(1, n_threads / D) : 0;
    const int rc = run_on_devices(std::vector<int>(devs.begin(), devs.begin() + D), [&](int k) {
        // the shard's own flat arrays: contigs, the reads its records use (first-use order), records, CIGARs
        const std::vector<int>& ids = shards[(size_t)k];
        std::vector<int64_t> c_off(1, 0), r_off(1, 0), cig_off(1, 0);
        std::vector<int32_t> rec_off(1, 0), rec_read, rec_pos;
        std::vector<uint8_t> rec_strand;
        std::vector<uint8_t, hs::NoInitAlloc<uint8_t>> c_seq, r_seq;
        std::vector<uint32_t, hs::NoInitAlloc<uint32_t>> cig;
        std::vector<int32_t> new_id((size_t)n_reads, -1);
        int n_sub_reads = 0;
        int64_t c_total = 0, r_total = 0, cig_total = 0, rec_total = 0;
        for (int c : ids) {
            c_total += h_contig_off[c + 1] - h_contig_off[c];
            for (int r = h_contig_rec_off[c]; r < h_contig_rec_off[c + 1]; ++r) {
                rec_total++; cig_total += h_rec_cig_off[r + 1] - h_rec_cig_off[r];
                if (new_id[(size_t)h_rec_read[r]] < 0) { new_id[(size_t)h_rec_read[r]] = n_sub_reads++; r_total += h_read_off[h_rec_read[r] + 1] - h_read_off[h_rec_read[r]]; }
            }
        }
        c_seq.resize((size_t)c_total); r_seq.resize((size_t)r_total); cig.resize((size_t)cig_total);
        rec_read.reserve((size_t)rec_total); rec_pos.reserve((size_t)rec_total); rec_strand.reserve((size_t)rec_total);
        r_off.assign((size_t)n_sub_reads + 1, 0);
        std::fill(new_id.begin(), new_id.end(), -1);
        n_sub_reads = 0;
        int64_t cw = 0, rw = 0, gw = 0;
        for (int c : ids) {
            const int64_t L = h_contig_off[c + 1] - h_contig_off[c];
            std::memcpy(c_seq.data() + cw, h_contig_seq + h_contig_off[c], (size_t)L); cw += L; c_off.push_back(cw);
            for (int r = h_contig_rec_off[c]; r < h_contig_rec_off[c + 1]; ++r) {
                const int g = h_rec_read[r];
                if (new_id[(size_t)g] < 0) {
                    new_id[(size_t)g] = n_sub_reads;
                    const int64_t n = h_read_off[g + 1] - h_read_off[g];
                    std::memcpy(r_seq.data() + rw, h_read_seq + h_read_off[g], (size_t)n); rw += n;
                    r_off[(size_t)++n_sub_reads] = rw;
                }
                rec_read.push_back(new_id[(size_t)g]); rec_pos.push_back(h_rec_pos[r]); rec_strand.push_back(h_rec_strand[r]);
                const int64_t n = h_rec_cig_off[r + 1] - h_rec_cig_off[r];
                std::memcpy(cig.data() + gw, h_cigar + h_rec_cig_off[r], (size_t)n * sizeof(uint32_t)); gw += n; cig_off.push_back(gw);
            }
            rec_off.push_back((int32_t)rec_read.size());
        }
        hs_cv_batch* b = nullptr;
        if (int rc2 = hs_cv_batch_create(c_seq.data(), c_off.data(), (int32_t)ids.size(), r_seq.data(), r_off.data(), n_sub_reads, rec_read.data(), rec_pos.data(),
                                         rec_strand.data(), cig_off.data(), cig.data(), rec_off.data(), &b)) return rc2;
        const int rc2 = hs_cv_run(b, automatic_snp_threshold, per, &parts[(size_t)k]);
        hs_cv_batch_destroy(b);
        return rc2;
    });
    if (rc) { for (hs_cv_result* r : parts) if (r) hs::free_cv_result(r); return rc; }
    std::vector<std::pair<int, int>> where((size_t)n_contigs);
    for (int k = 0; k < D; ++k) for (size_t i = 0; i < shards[(size_t)k].size(); ++i) where[(size_t)shards[(size_t)k][i]] = std::make_pair(k, (int)i);
    hs_cv_result* R = (hs_cv_result*)std::calloc(1, sizeof(hs_cv_result));
    int64_t S = 0, E = 0;
    for (hs_cv_result* r : parts) { S += r->snp_off[r->n_contigs]; E += r->col_off[r->snp_off[r->n_contigs]]; }
    R->n_contigs = n_contigs;
    R->mean_distance = (float*)std::malloc(std::max<size_t>(1, (size_t)n_contigs) * sizeof(float));
    R->depth = (float*)std::malloc(std::max<size_t>(1, (size_t)n_contigs) * sizeof(float));
    R->snp_off = (int64_t*)std::malloc(((size_t)n_contigs + 1) * sizeof(int64_t));
    R->snp_pos = (int32_t*)std::malloc(std::max<int64_t>(1, S) * sizeof(int32_t));
    R->snp_ref = (uint8_t*)std::malloc(std::max<int64_t>(1, S));
    R->snp_alt = (uint8_t*)std::malloc(std::max<int64_t>(1, S));
    R->snp_n_ref = (int32_t*)std::malloc(std::max<int64_t>(1, S) * sizeof(int32_t));
    R->snp_n_alt = (int32_t*)std::malloc(std::max<int64_t>(1, S) * sizeof(int32_t));
    R->col_off = (int64_t*)std::malloc(((size_t)S + 1) * sizeof(int64_t));
    R->col_idx = (int32_t*)std::malloc(std::max<int64_t>(1, E) * sizeof(int32_t));
    R->col_code = (uint8_t*)std::malloc(std::max<int64_t>(1, E));
    // contig order: where every contig's SNPs and column entries go (prefix sums over the contigs), then the copies on all host threads
    R->snp_off[0] = 0; R->col_off[0] = 0;
    std::vector<int64_t> ent0((size_t)n_contigs + 1, 0);
    for (int c = 0; c < n_contigs; ++c) {
        const hs_cv_result* r = parts[(size_t)where[(size_t)c].first];
        const int i = where[(size_t)c].second;
        R->mean_distance[c] = r->mean_distance[i]; R->depth[c] = r->depth[i];
        R->snp_off[c + 1] = R->snp_off[c] + (r->snp_off[i + 1] - r->snp_off[i]);
        ent0[(size_t)c + 1] = ent0[(size_t)c] + (r->col_off[r->snp_off[i + 1]] - r->col_off[r->snp_off[i]]);
    }
    R->col_off[S] = E;
    hs::hs_parallel_for(n_contigs, host_threads(), [&](int c) {
        const hs_cv_result* r = parts[(size_t)where[(size_t)c].first];
        const int i = where[(size_t)c].second;
        const int64_t q0 = r->snp_off[i], nq = r->snp_off[i + 1] - q0, s0 = R->snp_off[c];
        if (nq == 0) return;
        std::memcpy(R->snp_pos + s0, r->snp_pos + q0, (size_t)nq * sizeof(int32_t));
        std::memcpy(R->snp_ref + s0, r->snp_ref + q0, (size_t)nq);
        std::memcpy(R->snp_alt + s0, r->snp_alt + q0, (size_t)nq);
        std::memcpy(R->snp_n_ref + s0, r->snp_n_ref + q0, (size_t)nq * sizeof(int32_t));
        std::memcpy(R->snp_n_alt + s0, r->snp_n_alt + q0, (size_t)nq * sizeof(int32_t));
        const int64_t shift = ent0[(size_t)c] - r->col_off[q0];
        for (int64_t q = 0; q < nq; ++q) R->col_off[s0 + q] = r->col_off[q0 + q] + shift;
        const int64_t ne = r->col_off[q0 + nq] - r->col_off[q0];
        std::memcpy(R->col_idx + ent0[(size_t)c], r->col_idx + r->col_off[q0], (size_t)ne * sizeof(int32_t));
        std::memcpy(R->col_code + ent0[(size_t)c], r->col_code + r->col_off[q0], (size_t)ne);
    });
    R->error_rate = hs::job_error_rate(R->mean_distance, n_contigs, &R->n_contigs_with_error_rate);      // (contig order)
    for (hs_cv_result* r : parts) {
        R->t_device_ms += r->t_device_ms; R->t_host_ms += r->t_host_ms;
        for (int k = 0; k < 4; ++k) R->t_kernel_ms[k] += r->t_kernel_ms[k];
        R->t_kernel_k4_ms += r->t_kernel_k4_ms;
        R->n_columns_extracted += r->n_columns_extracted; R->n_columns_downloaded += r->n_columns_downloaded; R->n_columns_downloaded_late += r->n_columns_downloaded_late;
        hs::free_cv_result(r);
    }
    *out = R;
    return HS_OK;
}

}  // extern "C"

