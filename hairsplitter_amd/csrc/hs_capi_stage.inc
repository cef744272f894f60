// hs_capi_stage.inc -- part of hs_capi.hip: the stage-level C ABI on one device (hs_cv_run, hs_cv_select / _run_range, hs_sr_run_cv ...)
// and the contig groups on persistent threads (hs_pipeline_*: select + run, the fused call, options).
extern "C" {

// the host-side description of a batch, built once (it was copied per call and contig group: 4.5 MB each); the ploidy follows
// hs_cv_batch_set_ploidy, which is not called while a run is in flight
static const hs::CvMeta& batch_meta(const hs_cv_batch* b) {
    std::call_once(b->meta_once, [b] {
        hs::CvMeta& meta = b->meta;
        meta.n_contigs = b->n_contigs; meta.n_rec = b->n_rec; meta.contig_off = b->contig_off; meta.contig_rec_off = b->contig_rec_off;
        meta.pile_off = b->pile_off; meta.total_len = b->total_len; meta.rec_pos = b->rec_pos; meta.rec_refspan = b->rec_refspan; meta.ploidy = b->ploidy;
        meta.rank_of = b->h_rank_of; meta.orig_of = b->h_orig_of;
    });
    return b->meta;
}

int hs_cv_batch_set_ploidy(hs_cv_batch* b, const int32_t* ploidy) {
    if (!b) { set_error("hs_cv_batch_set_ploidy: null batch"); return HS_EINVAL; }
    if (ploidy) b->ploidy.assign(ploidy, ploidy + b->n_contigs); else b->ploidy.clear();
    (void)batch_meta(b);
    b->meta.ploidy = b->ploidy;
    return HS_OK;
}

int hs_cv_run(hs_cv_batch* b, float automatic_snp_threshold, int32_t n_threads, hs_cv_result** out) {
    if (int rc = require_device()) return rc;
    if (!b || !out) { set_error("hs_cv_run: null argument"); return HS_EINVAL; }
    if (int rc = bind_device(b->device)) return rc;
    const hs::CvMeta& meta = batch_meta(b);
    HipCvOps ops(b);
    return hs::cv_run(ops, meta, automatic_snp_threshold, n_threads, out);
}

int hs_read_graphs(const int32_t* d_sim, const int32_t* d_diff, const int64_t* ctg_out_off, const int32_t* ctg_n_reads,
                   int32_t n_contigs, const int32_t* win_contig, const int64_t* win_mask_off, const int32_t* mask_ids,
                   int32_t n_windows, float error_rate, int64_t** nbr_off, int32_t** nbr, int64_t* n_rows_host, void* stream) {
    if (int rc = require_device()) return rc;
    if (!nbr_off || !nbr || n_windows < 0 || n_contigs < 0) { set_error("hs_read_graphs: bad arguments"); return HS_EINVAL; }
    hs::SrWindowSet ws;
    ws.error_rate = error_rate;
    ws.win_contig.assign(win_contig, win_contig + n_windows);
    ws.win_row0.assign(win_mask_off, win_mask_off + n_windows + 1);
    ws.mask_ids.assign(mask_ids, mask_ids + win_mask_off[n_windows]);
    ws.n_dev_windows = n_windows;
    ws.win_final_empty.assign((size_t)n_windows, 0);
    ws.ctg_rank_off.assign((size_t)n_contigs, 0);
    int64_t ro = 0;
    for (int c = 0; c < n_contigs; ++c) { ws.ctg_rank_off[(size_t)c] = ro; ro += ctg_n_reads[c]; }
    ws.rank.resize((size_t)ro);         // the visiting order is of no interest here: the identity permutation per contig
    for (int c = 0; c < n_contigs; ++c) for (int32_t r = 0; r < ctg_n_reads[c]; ++r) ws.rank[(size_t)(ws.ctg_rank_off[(size_t)c] + r)] = r;
    for (int w = 0; w < n_windows; ++w) if (win_contig[w] < 0 || win_contig[w] >= n_contigs) { set_error("hs_read_graphs: window contig out of range"); return HS_EINVAL; }
    GraphRows G;
    float ms = 0;
    int64_t on_host = 0;
    if (int rc = graph_rows_build(d_sim, d_diff, std::vector<int64_t>(ctg_out_off, ctg_out_off + n_contigs), std::vector<int32_t>(ctg_n_reads, ctg_n_reads + n_contigs),
                                  ws, G, (hipStream_t)stream, &on_host, &ms)) return rc;
    *nbr_off = (int64_t*)std::malloc(((size_t)G.rows + 1) * sizeof(int64_t));
    *nbr = (int32_t*)std::malloc(((size_t)G.total + 1) * sizeof(int32_t));
    if (!*nbr_off || !*nbr) { set_error("hs_read_graphs: out of memory"); return HS_EINVAL; }
    if (int rc = d2h_pinned(*nbr_off, G.d_off.p, ((size_t)G.rows + 1) * 8, (hipStream_t)stream)) return rc;
    if (G.total > 0) { if (int rc = d2h_pinned(*nbr, G.d_nbr.p, (size_t)G.total * 4, (hipStream_t)stream)) return rc; }
    // the device keeps neighbours as window-local indices; this entry point reports read ids
    for (int w = 0; w < n_windows; ++w)
        for (int64_t e = (*nbr_off)[win_mask_off[w]]; e < (*nbr_off)[win_mask_off[w + 1]]; ++e) (*nbr)[e] = mask_ids[win_mask_off[w] + (*nbr)[e]];
    if (n_rows_host) *n_rows_host = on_host;
    return HS_OK;
}

int hs_cv_select(hs_cv_batch* b, hs_cv_selection** out) {
    if (int rc = require_device()) return rc;
    if (!b || !out) { set_error("hs_cv_select: null argument"); return HS_EINVAL; }
    if (int rc = bind_device(b->device)) return rc;
    const hs::CvMeta& meta = batch_meta(b);
    HipCvOps ops(b);
    hs::CvSelection* sel = new hs::CvSelection();
    if (int rc = hs::cv_pileup(ops, meta, *sel)) { delete sel; return rc; }
    hs_cv_selection* o = (hs_cv_selection*)std::calloc(1, sizeof(hs_cv_selection));
    o->n_selected = 0;
    for (int k = 0; k < 4; ++k) o->t_kernel_ms[k] = sel->k_ms[k];
    o->t_device_ms = sel->t_device_ms; o->t_host_ms = sel->t_host_ms;
    o->impl = sel;
    *out = o;
    return HS_OK;
}
void hs_cv_selection_destroy(hs_cv_selection* s) {
    if (!s) return;
    delete (hs::CvSelection*)s->impl;
    std::free(s);
}
int hs_cv_run_range(hs_cv_batch* b, const hs_cv_selection* sel, int32_t c0, int32_t c1, float automatic_snp_threshold, int32_t n_threads,
                    hs_cv_result** out) {
    if (int rc = require_device()) return rc;
    if (!b || !sel || !sel->impl || !out) { set_error("hs_cv_run_range: null argument"); return HS_EINVAL; }
    if (int rc = bind_device(b->device)) return rc;
    const hs::CvMeta& meta = batch_meta(b);
    HipCvOps ops(b);
    return hs::cv_run_range(ops, meta, ((const hs::CvSelection*)sel->impl)->rec_stats, c0, c1, automatic_snp_threshold, n_threads, out);
}

int hs_sr_run_cv_range(const hs_cv_batch* b, int32_t c0, int32_t c1, const hs_cv_result* cv, float error_rate, float rarest_strain_abundance,
                       int32_t low_memory, int32_t amplicon, uint32_t seed, int32_t n_threads, int32_t window_size, hs_sr_result** out) {
    if (int rc = require_device()) return rc;
    if (!b || !cv || !out) { set_error("hs_sr_run_cv_range: null argument"); return HS_EINVAL; }
    if (int rc = bind_device(b->device)) return rc;
    const hs::CvMeta& meta = batch_meta(b);
    HipSrOps ops;
    return hs::sr_run_from_cv(ops, meta, c0, c1, cv, error_rate, rarest_strain_abundance, low_memory, amplicon, seed, n_threads, window_size, out);
}
int hs_sr_run_cv(const hs_cv_batch* b, const hs_cv_result* cv, float error_rate, float rarest_strain_abundance, int32_t low_memory,
                 int32_t amplicon, uint32_t seed, int32_t n_threads, int32_t window_size, hs_sr_result** out) {
    if (!b) { set_error("hs_sr_run_cv: null argument"); return HS_EINVAL; }
    return hs_sr_run_cv_range(b, 0, b->n_contigs, cv, error_rate, rarest_strain_abundance, low_memory, amplicon, seed, n_threads, window_size, out);
}

// ---- contig groups on persistent threads (see the header) ----
struct hs_pipeline {
    hs_cv_batch* batch = nullptr;
    std::vector<std::pair<int, int>> ranges;
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    std::function<int(int)> job;
    std::function<void()> on_fail;      // called by a group thread whose job failed (or that never bound to the device): releases whoever waits for that group
    uint64_t gen = 0;
    int pending = 0;
    bool quit = false;
    std::vector<int> rcs;
    std::vector<std::string> errs;
    hs_cv_selection* sel = nullptr;
    std::vector<hs_cv_result*> cv;
    std::vector<hs::SrWorkspace> sr_keep;      // per group: the stage-4 plans and visiting orders live from step to step
    std::vector<std::unique_ptr<HipCvOps::Keep>> cv_keep;      // per group: the sizes of its column pass (the next step queues it without asking)
    std::vector<HipSrOps::Keep> sr_dev_keep;
    HipCvOps::K2Order k2_order;
    bool keep_columns = false;      // HS_PIPELINE_KEEP_COLUMNS
    bool sparse_labels = false;     // HS_PIPELINE_SPARSE_LABELS: the labels per window as (reads of the window, their labels), no dense array
    std::vector<int64_t> sp_off; std::vector<int32_t> sp_ids, sp_labels;      // (the last call's, contig order: hs_pipeline_sparse_labels)
    bool alleles = false;           // HS_PIPELINE_ALLELES: every group crosses its labels with its SNP columns at the end of its chain
    hs_allele_table* allele_table = nullptr;      // (the last call's, contig order: hs_pipeline_alleles)
    bool recruit = false;           // HS_PIPELINE_RECRUIT: every group also recruits its windows' unlabelled reads behind its allele cells
    hs_recruit_params recruit_params = hs_recruit_params_default();
    hs_recruit_table* recruit_table = nullptr;    // (the last call's, contig order: hs_pipeline_recruits)

    int device = 0;        // = batch->device: the group threads bind themselves to it (a new thread starts on device 0)
    std::vector<int> thread_device;   // what every group thread found current after binding (hs_pipeline_thread_devices)
    void worker(int g) {
        ::prctl(PR_SET_NAME, "hs-group", 0, 0, 0);
        uint64_t seen = 0;
        const bool bound = hipSetDevice(device) == hipSuccess;
        { int cur = -1; if (!bound || hipGetDevice(&cur) != hipSuccess) cur = -1; std::lock_guard<std::mutex> lk(mu); thread_device[(size_t)g] = cur; }
        for (;;) {
            std::function<int(int)> f;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return quit || gen != seen; });
                if (quit) return;
                seen = gen; f = job;
            }
            int rc;
            if (!bound) { set_error("a contig-group thread could not bind to the device of its batch"); rc = HS_EHIP; }
            else rc = f(g);
            if (rc) { k2_order.abort(); std::function<void()> h; { std::lock_guard<std::mutex> lk(mu); h = on_fail; } if (h) h(); }      // (nobody waits for a group that is gone: its turn, its share of the error rate)
            {
                std::lock_guard<std::mutex> lk(mu);
                rcs[(size_t)g] = rc;
                if (rc) errs[(size_t)g] = hs_last_error();
                if (--pending == 0) cv_done.notify_one();
            }
        }
    }
    int run(const std::function<int(int)>& f) {   // f(group) on every group thread; first failure wins
        {
            std::lock_guard<std::mutex> lk(mu);
            job = f; pending = (int)threads.size(); gen++;
        }
        cv_go.notify_all();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
        for (size_t g = 0; g < rcs.size(); ++g) if (rcs[g]) { set_error(errs[g]); return rcs[g]; }
        return HS_OK;
    }
    std::vector<std::unique_ptr<HBuf>> entry_blocks;      // per group: the pinned block the current result's column entries lie in
    void drop_cv() {
        for (hs_cv_result*& r : cv) { if (r) hs::free_cv_result(r); r = nullptr; }
        for (auto& h : entry_blocks) if (h) h->release();
        if (sel) { hs_cv_selection_destroy(sel); sel = nullptr; }
    }
};

int hs_pipeline_create(hs_cv_batch* b, int32_t n_groups, hs_pipeline** out) {
    if (int rc = require_device()) return rc;
    if (!b || !out) { set_error("hs_pipeline_create: null argument"); return HS_EINVAL; }
    tune_allocator();
    hs_pipeline* p = new hs_pipeline();
    p->batch = b;
    const int C = b->n_contigs;
    const int G = std::max(1, std::min<int>(n_groups, std::max(C, 1)));
    {
        // consecutive contigs per group, cut where the aligned bases (= pileup bytes) reach g / G of the batch: the groups' chains are
        // as long as their data, and the longest one ends the step
        std::vector<int> cut((size_t)G + 1, 0);
        cut[(size_t)G] = C;
        const int64_t total = b->pile_off.empty() ? 0 : b->pile_off.back();
        if (total > 0 && (int)b->contig_rec_off.size() == C + 1) {
            // The groups reach the host one after the other (the device hands out their candidate columns about 0.8 ms apart, K2 by K2),
            // and the step ends when the LAST group's chain -- loops A / B, K4, all of stage 4 -- is through: the later a group starts,
            // the smaller it is made, so that the chains end together. HS_GROUP_TAPER = share of the last group relative to the first
            // (1 = equal groups), linear in between. Default 0.5: with the groups' K2 launches in group order on the device (K2Turn) the same box,
            // alternating runs, 500-contig job: 16.6 / 16.3 / 16.5 ms per step against 17.4 / 16.9 / 17.5 with equal groups; 0.3: 16.3 / 16.6.
            // With few groups the FIRST group's chain is the long one (two groups start almost together): the default runs from equal
            // groups at G = 2 to 0.5 at G >= 8 (a rank of 8 with two groups: 7.2 ms per step with 0.5, its first group's loops A / B 2.9 ms on three threads).
            static const double taper_env = []() { const char* e = std::getenv("HS_GROUP_TAPER"); const double v = e ? std::atof(e) : 0.0; return v > 0 && v <= 1 ? v : 0.0; }();
            const double taper = taper_env > 0 ? taper_env : 1.0 - 0.5 * std::min(1.0, std::max(0.0, (G - 2) / 6.0));
            std::vector<double> upto((size_t)G + 1, 0.0);
            for (int g = 0; g < G; ++g) upto[(size_t)g + 1] = upto[(size_t)g] + (G > 1 ? 1.0 + (taper - 1.0) * g / (G - 1) : 1.0);
            int c = 0;
            for (int g = 1; g < G; ++g) {
                const int64_t want = (int64_t)((double)total * upto[(size_t)g] / upto[(size_t)G]);
                while (c < C && b->pile_off[(size_t)b->contig_rec_off[(size_t)c + 1]] <= want) ++c;
                // the contig that crosses the mark goes to the side it lies more on
                if (c < C) {
                    const int64_t lo = b->pile_off[(size_t)b->contig_rec_off[(size_t)c]], hi = b->pile_off[(size_t)b->contig_rec_off[(size_t)c + 1]];
                    if (hi - want < want - lo) ++c;
                }
                cut[(size_t)g] = std::max(cut[(size_t)g - 1], std::min(c, C));
            }
        } else for (int g = 1; g < G; ++g) cut[(size_t)g] = (int)((int64_t)C * g / G);
        // every group keeps at least one contig while there are enough of them
        for (int g = 1; g < G; ++g) cut[(size_t)g] = std::max(cut[(size_t)g], std::min(g, C));
        for (int g = G - 1; g >= 1; --g) cut[(size_t)g] = std::min(cut[(size_t)g], C - (G - g));
        for (int g = 1; g < G; ++g) cut[(size_t)g] = std::max(cut[(size_t)g], cut[(size_t)g - 1]);
        for (int g = 0; g < G; ++g) p->ranges.push_back(std::make_pair(cut[(size_t)g], cut[(size_t)g + 1]));
    }
    p->rcs.assign((size_t)G, 0); p->errs.assign((size_t)G, std::string()); p->cv.assign((size_t)G, nullptr);
    p->device = b->device; p->thread_device.assign((size_t)G, -1);
    p->sr_keep.resize((size_t)G);
    for (int g = 0; g < G; ++g) p->entry_blocks.emplace_back(new HBuf());
    for (int g = 0; g < G; ++g) p->cv_keep.emplace_back(new HipCvOps::Keep());
    p->sr_dev_keep.resize((size_t)G);
    for (int g = 0; g < G; ++g) p->threads.emplace_back([p, g] { p->worker(g); });
    *out = p;
    return HS_OK;
}

int hs_cv_batch_device(const hs_cv_batch* b) { return b ? b->device : -1; }
int hs_pipeline_set_option(hs_pipeline* p, int32_t option, int64_t value) {
    if (!p) { set_error("hs_pipeline_set_option: null pipeline"); return HS_EINVAL; }
    if (option == HS_PIPELINE_KEEP_COLUMNS) { p->keep_columns = value != 0; return HS_OK; }
    if (option == HS_PIPELINE_SPARSE_LABELS) { p->sparse_labels = value != 0; return HS_OK; }
    if (option == HS_PIPELINE_ALLELES) { p->alleles = value != 0; return HS_OK; }
    if (option == HS_PIPELINE_RECRUIT) { p->recruit = value != 0; return HS_OK; }
    set_error("hs_pipeline_set_option: unknown option"); return HS_EINVAL;
}
int hs_pipeline_groups(const hs_pipeline* p) { return p ? (int)p->ranges.size() : 0; }
int hs_pipeline_group_range(const hs_pipeline* p, int32_t g, int32_t* c0, int32_t* c1) {
    if (!p || g < 0 || g >= (int32_t)p->ranges.size()) { set_error("hs_pipeline_group_range: no such group"); return HS_EINVAL; }
    if (c0) *c0 = p->ranges[(size_t)g].first; if (c1) *c1 = p->ranges[(size_t)g].second;
    return HS_OK;
}
int hs_pipeline_sparse_labels(const hs_pipeline* p, const int64_t** win_row_off, const int32_t** ids, const int32_t** labels, int64_t* n_windows, int64_t* n_rows) {
    if (!p || p->sp_off.empty()) { set_error("hs_pipeline_sparse_labels: no call with HS_PIPELINE_SPARSE_LABELS yet"); return HS_EINVAL; }
    if (win_row_off) *win_row_off = p->sp_off.data(); if (ids) *ids = p->sp_ids.data(); if (labels) *labels = p->sp_labels.data();
    if (n_windows) *n_windows = (int64_t)p->sp_off.size() - 1; if (n_rows) *n_rows = p->sp_off.back();
    return HS_OK;
}
const hs_allele_table* hs_pipeline_alleles(const hs_pipeline* p) { return p ? p->allele_table : nullptr; }
const hs_recruit_table* hs_pipeline_recruits(const hs_pipeline* p) { return p ? p->recruit_table : nullptr; }
int hs_pipeline_set_recruit_params(hs_pipeline* p, const hs_recruit_params* params) {
    if (!p || !params || !hs::recruit_params_valid(*params)) { set_error("hs_pipeline_set_recruit_params: null argument or thresholds out of range"); return HS_EINVAL; }
    p->recruit_params = *params;
    return HS_OK;
}
const hs_cv_result* hs_pipeline_group_cv(const hs_pipeline* p, int32_t g) { return (p && g >= 0 && g < (int32_t)p->cv.size()) ? p->cv[(size_t)g] : nullptr; }
// the device every contig-group thread is bound to (-1: not bound yet / failed); returns the number of groups
int hs_pipeline_thread_devices(hs_pipeline* p, int32_t* out, int32_t cap) {
    if (!p) return 0;
    // the threads bind themselves when they start: an empty job makes sure every one of them has got that far
    (void)p->run([](int) { return HS_OK; });
    std::lock_guard<std::mutex> lk(p->mu);
    for (size_t g = 0; g < p->thread_device.size() && (int32_t)g < cap; ++g) out[g] = p->thread_device[g];
    return (int)p->thread_device.size();
}

void hs_pipeline_destroy(hs_pipeline* p) {
    if (!p) return;
    { std::lock_guard<std::mutex> lk(p->mu); p->quit = true; }
    p->cv_go.notify_all();
    for (std::thread& t : p->threads) t.join();
    (void)bind_device(p->device);
    p->drop_cv();
    hs::alleles_free(p->allele_table);
    hs::recruit_free(p->recruit_table);
    delete p;
}

static hs_sr_result* concat_sr_parts(hs_pipeline* p, std::vector<hs_sr_result*>& parts, const std::vector<hs::SrSparseLabels>& sparse, hs_pipeline_stats* st) {
    // concatenate in contig order
    hs_sr_result* R = (hs_sr_result*)std::calloc(1, sizeof(hs_sr_result));
    int64_t W = 0, NL = 0;
    for (hs_sr_result* r : parts) { W += r->win_off[r->n_contigs]; NL += r->label_off[r->win_off[r->n_contigs]]; }
    R->n_contigs = p->batch->n_contigs;
    R->win_off = (int64_t*)std::malloc(((size_t)R->n_contigs + 1) * sizeof(int64_t));
    R->win_start = (int32_t*)std::malloc((size_t)std::max<int64_t>(1, W) * sizeof(int32_t));
    R->win_end = (int32_t*)std::malloc((size_t)std::max<int64_t>(1, W) * sizeof(int32_t));
    R->label_off = (int64_t*)std::malloc(((size_t)W + 1) * sizeof(int64_t));
    R->labels = p->sparse_labels ? nullptr : hs::sr_labels_alloc((size_t)NL);
    int64_t w0 = 0, l0 = 0; int c0 = 0;
    R->win_off[0] = 0; R->label_off[0] = 0;
    std::vector<int64_t> part_l0(parts.size(), 0);
    for (size_t pi = 0; pi < parts.size(); ++pi) {
        hs_sr_result* r = parts[pi];
        const int64_t w = r->win_off[r->n_contigs], nl = r->label_off[w];
        for (int c = 0; c < r->n_contigs; ++c) R->win_off[c0 + c + 1] = w0 + r->win_off[c + 1];
        if (w) { std::memcpy(R->win_start + w0, r->win_start, (size_t)w * sizeof(int32_t)); std::memcpy(R->win_end + w0, r->win_end, (size_t)w * sizeof(int32_t)); }
        for (int64_t k = 0; k < w; ++k) R->label_off[w0 + k + 1] = l0 + r->label_off[k + 1];
        part_l0[pi] = l0;
        R->t_device_ms += r->t_device_ms; R->t_host_ms += r->t_host_ms; R->n_cw_instances += r->n_cw_instances;
        for (int k = 0; k < 4; ++k) R->t_kernel_ms[k] += r->t_kernel_ms[k];
        R->t_kernel_graph_ms += r->t_kernel_graph_ms; R->n_graph_rows_host += r->n_graph_rows_host; R->n_windows_finished_on_host += r->n_windows_finished_on_host;
        R->n_cw_sweeps += r->n_cw_sweeps; R->cw_bytes += r->cw_bytes; R->graph_nnz += r->graph_nnz; R->n_graph_rows += r->n_graph_rows; R->simdiff_bytes += r->simdiff_bytes;
        w0 += w; l0 += nl; c0 += r->n_contigs;
    }
    if (p->sparse_labels) {
        // what the .gro lists and nothing else: per window its reads and their labels, the groups' lists one after the other in contig order
        size_t rows = 0;
        std::vector<size_t> part_r0(parts.size(), 0), part_w0(parts.size(), 0);
        { size_t w = 0; for (size_t pi = 0; pi < parts.size(); ++pi) { part_r0[pi] = rows; part_w0[pi] = w; rows += sparse[pi].ids.size(); w += sparse[pi].off.size() - 1; } }
        p->sp_off.resize((size_t)W + 1); p->sp_ids.resize(rows); p->sp_labels.resize(rows);
        hs::hs_parallel_for((int)parts.size(), host_threads(), [&](int pi) {
            const hs::SrSparseLabels& sp = sparse[(size_t)pi];
            for (size_t w = 0; w + 1 < sp.off.size(); ++w) p->sp_off[part_w0[(size_t)pi] + w] = (int64_t)part_r0[(size_t)pi] + sp.off[w];
            if (!sp.ids.empty()) { std::memcpy(p->sp_ids.data() + part_r0[(size_t)pi], sp.ids.data(), sp.ids.size() * 4); std::memcpy(p->sp_labels.data() + part_r0[(size_t)pi], sp.labels.data(), sp.labels.size() * 4); }
        });
        p->sp_off[(size_t)W] = (int64_t)rows;
    } else {
    // the labels (tens of MB per batch) are spread over the reads of every window here, once, in their final place: blocks of
    // windows on the caller's worker threads
    {
        struct Blk { int part; int64_t w0, w1; };
        std::vector<Blk> blks;
        for (size_t pi = 0; pi < parts.size(); ++pi) {
            const int64_t w = parts[pi]->win_off[parts[pi]->n_contigs];
            for (int64_t a = 0; a < w; a += 64) blks.push_back(Blk{(int)pi, a, std::min<int64_t>(w, a + 64)});
        }
        hs::hs_parallel_for((int)blks.size(), host_threads(), [&](int i) {
            const Blk& b = blks[(size_t)i];
            const hs_sr_result* r = parts[(size_t)b.part];
            hs::sr_expand_labels(sparse[(size_t)b.part], r->label_off, b.w0, b.w1, R->labels + part_l0[(size_t)b.part]);
        });
    }
    }
    for (hs_sr_result* r : parts) hs::free_sr_result(r);
    if (st) {
        st->n_cw_instances = R->n_cw_instances; st->n_graph_rows_host = R->n_graph_rows_host;
        st->t_device_ms += R->t_device_ms; st->t_host_ms += R->t_host_ms;
        for (int k = 0; k < 4; ++k) st->t_kernel_sr_ms[k] = R->t_kernel_ms[k];
        st->t_kernel_graph_ms = R->t_kernel_graph_ms;
        st->n_cw_sweeps = R->n_cw_sweeps; st->cw_bytes = R->cw_bytes; st->graph_nnz = R->graph_nnz; st->n_graph_rows = R->n_graph_rows; st->simdiff_bytes = R->simdiff_bytes;
    }
    return R;
}

// ---- test taps of the column pass (include/hairsplitter_hip.h: hs_cv_taps) ----
void hs_cv_taps_destroy(hs_cv_taps* t) {
    if (!t) return;
    std::free(t->col_gpos); std::free(t->col_rec); std::free(t->col_off); std::free(t->col_idx); std::free(t->col_code); std::free(t->cand_rec); std::free(t->cand_col);
    std::free(t->cand_bits); std::free(t->cand_words); std::free(t->contig_n_cand); std::free(t->contig_mean_distance);
    std::free(t);
}
int hs_cv_column_pass_taps(hs_cv_batch* b, int32_t c0, int32_t c1, float automatic_snp_threshold, hs_cv_taps** out) {
    if (int rc = require_device()) return rc;
    if (!b || !out || c0 < 0 || c1 > b->n_contigs || c0 > c1) { set_error("hs_cv_column_pass_taps: bad arguments"); return HS_EINVAL; }
    static_assert(sizeof(hs_cand_bits) == sizeof(hs::CandBits), "hs_cand_bits layout");
    if (int rc = bind_device(b->device)) return rc;
    HipCvOps ops(b);
    ops.own_pileup = true;      // the range brings up its own share of the pileup, as a contig group of the pipeline does
    hs::CvCandidates cand;
    float k_ms[3];
    const std::vector<int32_t> no_min_reads;
    if (int rc = ops.extract_candidates(c0, c1, no_min_reads, automatic_snp_threshold, cand, k_ms, true)) return rc;
    hs_cv_taps* t = (hs_cv_taps*)std::calloc(1, sizeof(hs_cv_taps));
    const int C = c1 - c0;
    t->n_contigs = C; t->n_cols = ops.n_cols; t->n_entries = ops.n_entries; t->n_cand = cand.n_cand;
    auto dup_d = [&](void** dst, const void* d, size_t bytes) -> int {
        *dst = std::malloc(std::max<size_t>(bytes, 16));
        if (!*dst) { set_error("hs_cv_column_pass_taps: out of memory"); return HS_EINVAL; }
        if (bytes) HS_HIP(hipMemcpy(*dst, d, bytes, hipMemcpyDeviceToHost));
        return HS_OK;
    };
    int rc = HS_OK;
    const size_t n = (size_t)t->n_cols, e = (size_t)t->n_entries, nc = (size_t)t->n_cand;
    if (!rc && n) rc = dup_d((void**)&t->col_gpos, ops.d_col_gpos.p, n * 8);
    if (!rc && n) rc = dup_d((void**)&t->col_rec, ops.d_col_rec.p, n * sizeof(hs_colrec));
    if (!rc) rc = n ? dup_d((void**)&t->col_off, ops.d_co.p, (n + 1) * 8) : dup_d((void**)&t->col_off, nullptr, 0);
    if (!rc && !n) t->col_off[0] = 0;
    if (!rc && e) rc = dup_d((void**)&t->col_idx, ops.d_ci.p, e * 4);
    if (!rc && e) rc = dup_d((void**)&t->col_code, ops.d_cc.p, e);
    if (!rc && nc) {
        const char* cb = (const char*)ops.d_cand_pk.p;
        rc = dup_d((void**)&t->cand_rec, cb + ops.cand_layout.rec, nc * sizeof(hs_colrec));
        if (!rc) rc = dup_d((void**)&t->cand_col, cb + ops.cand_layout.col, nc * 4);
        if (!rc) {
            t->n_cand_words = ops.cand_bits_words();
            t->cand_bits = (hs_cand_bits*)std::malloc(nc * sizeof(hs_cand_bits));
            t->cand_words = (uint64_t*)std::malloc(std::max<size_t>(16, (size_t)t->n_cand_words * 8));
            if (!t->cand_bits || !t->cand_words || !cand.bits) { set_error("hs_cv_column_pass_taps: no bit sets"); rc = HS_EINVAL; }
            else { std::memcpy(t->cand_bits, cand.bits, nc * sizeof(hs_cand_bits)); std::memcpy(t->cand_words, cand.words, (size_t)t->n_cand_words * 8); }
        }
    }
    if (!rc) {
        t->contig_n_cand = (int32_t*)std::malloc(std::max<size_t>(16, (size_t)C * 4));
        t->contig_mean_distance = (float*)std::malloc(std::max<size_t>(16, (size_t)C * 4));
        if (C) { std::memcpy(t->contig_n_cand, cand.contig_n_cand.data(), (size_t)C * 4); std::memcpy(t->contig_mean_distance, cand.contig_mean_distance.data(), (size_t)C * 4); }
    }
    if (rc) { hs_cv_taps_destroy(t); return rc; }
    *out = t;
    return HS_OK;
}

// ---- test tap of the pileup as a contig group launches it (include/hairsplitter_hip.h: hs_cv_pileup_taps) ----
void hs_cv_pileup_tap_destroy(hs_cv_pileup_taps* t) {
    if (!t) return;
    std::free(t->pile); std::free(t->pile_addr); std::free(t->rec_stats); std::free(t->rec_chunk_off); std::free(t->chunk_table);
    std::free(t);
}
int hs_cv_pileup_tap(hs_cv_batch* b, int32_t c0, int32_t c1, int32_t fill, hs_cv_pileup_taps** out) {
    if (int rc = require_device()) return rc;
    if (!b || !out || c0 < 0 || c1 > b->n_contigs || c0 > c1 || fill < 0 || fill > 255) { set_error("hs_cv_pileup_tap: bad arguments"); return HS_EINVAL; }
    if (int rc = bind_device(b->device)) return rc;
    HipCvOps ops(b);
    ops.own_pileup = true;
    const size_t n_rec = (size_t)b->n_rec;
    DBuf d_md, d_min_reads;      // what k_contig_error leaves behind the pileup of a group
    if (int rc = d_md.alloc(std::max<size_t>(1, (size_t)(c1 - c0)) * 4)) return rc;
    if (int rc = d_min_reads.alloc(std::max<size_t>(1, (size_t)(c1 - c0)) * 4)) return rc;
    HS_HIP(hipMemsetAsync(b->pile.p, fill, b->pile.bytes, ops.stream));
    if (b->rec_stats.bytes) HS_HIP(hipMemsetAsync(b->rec_stats.p, 0xFF, b->rec_stats.bytes, ops.stream));
    if (b->chunk_scratch.bytes) HS_HIP(hipMemsetAsync(b->chunk_scratch.p, 0xFF, b->chunk_scratch.bytes, ops.stream));
    if (c1 > c0) { if (int rc = ops.pileup_range_launch(c0, c1, d_md.as<float>(), d_min_reads.as<int32_t>(), 3)) return rc; }
    HS_HIP(hipStreamSynchronize(ops.stream));
    ops.kc.flush();
    hs_cv_pileup_taps* t = (hs_cv_pileup_taps*)std::calloc(1, sizeof(hs_cv_pileup_taps));
    if (!t) { set_error("hs_cv_pileup_tap: out of memory"); return HS_EINVAL; }
    t->n_rec = b->n_rec;
    t->pile_lead = (int32_t)(b->pile_ptr() - b->pile.as<uint8_t>());
    t->pile_alloc_bytes = (int64_t)b->pile.bytes;
    t->n_chunks = (int64_t)(b->chunk_scratch.bytes / 16);
    auto dup_d = [&](void** dst, const void* d, size_t bytes) -> int {
        *dst = std::malloc(std::max<size_t>(bytes, 16));
        if (!*dst) { set_error("hs_cv_pileup_tap: out of memory"); return HS_EINVAL; }
        if (bytes) HS_HIP(hipMemcpy(*dst, d, bytes, hipMemcpyDeviceToHost));
        return HS_OK;
    };
    int rc = dup_d((void**)&t->pile, b->pile.p, b->pile.bytes);
    if (!rc) rc = dup_d((void**)&t->rec_stats, b->rec_stats.p, n_rec * 16);
    if (!rc) rc = dup_d((void**)&t->rec_chunk_off, b->rec_chunk_off.p, (n_rec + 1) * 8);
    if (!rc) rc = dup_d((void**)&t->chunk_table, b->chunk_scratch.p, b->chunk_scratch.bytes);
    if (!rc) {
        t->pile_addr = (int64_t*)std::malloc((n_rec + 1) * 8);
        if (!t->pile_addr) { set_error("hs_cv_pileup_tap: out of memory"); rc = HS_EINVAL; }
        else std::memcpy(t->pile_addr, b->pile_addr.data(), (n_rec + 1) * 8);
    }
    if (rc) { hs_cv_pileup_tap_destroy(t); return rc; }
    *out = t;
    return HS_OK;
}

int hs_pipeline_select(hs_pipeline* p, float* mean_distance, hs_pipeline_stats* st) {
    if (!p || !mean_distance) { set_error("hs_pipeline_select: null argument"); return HS_EINVAL; }
    if (int rc = bind_device(p->batch->device)) return rc;
    timing_next_step();      // (a step of the two-call form begins here)
    p->drop_cv();
    if (int rc = hs_cv_select(p->batch, &p->sel)) return rc;
    const hs::CvSelection& sel = *(const hs::CvSelection*)p->sel->impl;
    const hs_cv_batch* b = p->batch;
    for (int c = 0; c < b->n_contigs; ++c) {   // call_variants.cpp:434 per contig, from the integer counters of K1
        int64_t nerr = 0, nlen = 0;
        for (int r = b->contig_rec_off[(size_t)c]; r < b->contig_rec_off[(size_t)c + 1]; ++r) { nerr += sel.rec_stats[(size_t)r * 4 + 1]; nlen += sel.rec_stats[(size_t)r * 4 + 2]; }
        mean_distance[c] = hs::mean_distance_from_counts(nerr, nlen);
    }
    if (st) {
        std::memset(st, 0, sizeof *st);
        st->t_device_ms = p->sel->t_device_ms; st->t_host_ms = p->sel->t_host_ms;
        st->t_kernel_cv_ms[0] = p->sel->t_kernel_ms[0]; st->t_kernel_cv_ms[3] = p->sel->t_kernel_ms[3];
    }
    return HS_OK;
}

// ---- the contig-group step behind hs_pipeline_run and hs_pipeline_run_fused ----

// n_threads <= 0: three workers per usable core over all groups -- a group is on the host for part of its chain only (the
// rest it waits for the device), so that many threads keep the cores busy without queueing behind each other (500-contig
// bench, 16 usable cores: 16 threads 74 ms per step, 32: 46, 48: 44, 64: 47, 128: 51)
static int pipeline_threads_per_group(int n_threads, int G) {
    if (n_threads <= 0) n_threads = 3 * host_threads();
    return std::max(1, n_threads / G);
}

// the window size over the WHOLE batch (hs_job_rules.h: window_size_from_counts looks at every read of every contig): READ
// limits are (POS-1, POS + reference span) (input_output.cpp:503-511); --amplicon: the longest contig
static int32_t pipeline_window_size(const hs_cv_batch* b, bool amplicon) {
    if (amplicon) { int32_t w = 0; for (int c = 0; c < b->n_contigs; ++c) w = std::max<int32_t>(w, (int32_t)(b->contig_off[(size_t)c + 1] - b->contig_off[(size_t)c])); return w; }
    uint32_t sum = 0; int64_t reads = 0, above = 0;
    for (int64_t v : b->rec_refspan) hs::window_size_count_read((int)v + 2, sum, reads, above);
    return hs::window_size_from_counts(sum, reads, above);
}

// what the groups' stage-3 results add to the statistics of a call
static void fold_cv_stats(hs_pipeline_stats* st, const hs_pipeline* p) {
    for (const hs_cv_result* r : p->cv) {
        st->n_snps += r->snp_off[r->n_contigs];
        st->t_device_ms += r->t_device_ms; st->t_host_ms += r->t_host_ms;
        st->t_kernel_cv_ms[2] += r->t_kernel_ms[2]; st->t_kernel_k4_ms += r->t_kernel_k4_ms;
        st->n_columns_extracted += r->n_columns_extracted; st->n_columns_downloaded += r->n_columns_downloaded;
        st->n_columns_downloaded_late += r->n_columns_downloaded_late;
        st->t_kernel_cv_ms[1] += r->t_kernel_ms[1];
    }
}

// The meeting point of the fused call's groups before stage 4: a group's mean distances are known (from the host's sums, or with
// its candidate columns from the device), the last group to get here forms the job's error rate (hs_job_rules.h), which is long
// before the first one needs it for stage 4; a group that fails releases the others.
struct GroupMeeting {
    std::mutex mu; std::condition_variable cv;
    int arrived = 0; bool aborted = false;
    std::vector<float> md;      // [n_contigs] what hs_pipeline_select would have returned
    float error_rate = 0;
    void arrive(const float* md_g, int c0, int c1, int G) {
        if (c1 > c0) std::memcpy(md.data() + c0, md_g, (size_t)(c1 - c0) * sizeof(float));
        std::lock_guard<std::mutex> lk(mu);
        if (++arrived == G) {
            error_rate = hs::error_rate_as_stage4_reads_it(hs::job_error_rate(md.data(), (int)md.size(), nullptr));
            cv.notify_all();
        }
    }
    void abort() { { std::lock_guard<std::mutex> lk(mu); aborted = true; } cv.notify_all(); }
    bool wait_for_all(int G) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return arrived == G || aborted; }); return !aborted; }
};

// one call's state, on the caller's stack
struct GroupCall {
    float automatic_snp_threshold, error_rate, rarest_strain_abundance;      // (error_rate: the caller's; the fused call's comes from `meet`)
    int32_t low_memory, amplicon; uint32_t seed; int per; int32_t window_size;
    std::vector<hs_sr_result*> parts;
    std::vector<hs::SrSparseLabels> sparse;      // the groups leave their labels per window; concat_sr_parts spreads them
    GroupMeeting* meet;      // the fused call only: its groups bring up their own share of the pileup and meet before stage 4
    std::vector<TablePair> tables;      // HS_PIPELINE_ALLELES, HS_PIPELINE_RECRUIT: the groups' shares of the two tables
};
// (error_rate: the two-call form's; meet: the fused call's)
static GroupCall group_call(const hs_pipeline* p, float automatic_snp_threshold, float error_rate, float rarest_strain_abundance, int32_t low_memory, int32_t amplicon,
                            uint32_t seed, int32_t n_threads, int32_t window_size, GroupMeeting* meet) {
    const size_t G = p->ranges.size();
    if (window_size <= 0) window_size = pipeline_window_size(p->batch, amplicon != 0);
    return GroupCall{automatic_snp_threshold, error_rate, rarest_strain_abundance, low_memory, amplicon, seed, pipeline_threads_per_group(n_threads, (int)G), window_size,
                     std::vector<hs_sr_result*>(G, nullptr), std::vector<hs::SrSparseLabels>(G), meet, std::vector<TablePair>(G)};
}

// the groups' shares of the allele table, contig order; the previous call's table goes
static int pipeline_merge_alleles(hs_pipeline* p, GroupCall& call) {
    hs::alleles_free(p->allele_table); p->allele_table = nullptr;
    hs::recruit_free(p->recruit_table); p->recruit_table = nullptr;
    std::vector<const hs_allele_table*> alleles; std::vector<const hs_recruit_table*> recruit;
    for (const TablePair& t : call.tables) { alleles.push_back(t.alleles.get()); recruit.push_back(t.recruit.get()); }
    if (p->recruit) {
        p->recruit_table = hs::recruit_concat(recruit);
        if (!p->recruit_table) { set_error("recruit table: out of memory"); return HS_EINVAL; }
    }
    if (!p->alleles) return HS_OK;
    p->allele_table = hs::alleles_concat(alleles);
    if (!p->allele_table) { set_error("allele table: out of memory"); return HS_EINVAL; }
    return HS_OK;
}

// Group g's chain: the column pass, stage 3's host glue, stage 4 on the columns where stage 3 packed them. Everything is queued
// on the thread's own stream (the null stream of HipCvOps / HipSrOps under -fgpu-default-stream=per-thread); a low-priority stream
// for the head of the chain and a high-priority one for the rest was measured in round 4: 24.2 ms per C4 step against 18.6, the
// low-priority heads are on the critical path of the groups that come later.
static int pipeline_group_step(hs_pipeline* p, GroupCall& call, int g) {
    const int c0 = p->ranges[(size_t)g].first, c1 = p->ranges[(size_t)g].second;
    const int G = (int)p->ranges.size();
    const int per = call.per;
    GroupMeeting* const meet = call.meet;
    hs_cv_result*& cv = p->cv[(size_t)g];
    const hs::CvMeta& meta = batch_meta(p->batch);
    HipCvOps cv_ops(p->batch);
    cv_ops.keep = p->cv_keep[(size_t)g].get(); cv_ops.k2_order = &p->k2_order; cv_ops.order_ticket = g;
    cv_ops.defer_entries = p->keep_columns;
    auto fail = [&](int r) { if (meet) meet->abort(); return r; };      // (the two-call form: the worker's k2_order.abort() is all a failing group owes the others)
    // the SNP columns stay on the device: stage 4 takes them over where stage 3 packed them (HS_COLUMNS_VIA_HOST=1: down and up again)
    static const bool via_host = std::getenv("HS_COLUMNS_VIA_HOST") != nullptr;
    const bool resident = !via_host && !p->keep_columns;
    if (cv) { hs::free_cv_result(cv); cv = nullptr; }      // (the two-call form: the previous call's; the fused call has dropped them all)
    float error_rate = call.error_rate;
    if (meet) {
        // the group's share of the pileup is the head of its column pass on the device (K0, K1, the contigs' distances, K2 ...): one chain,
        // queued behind the previous group's, no host wait before the candidates
        cv_ops.own_pileup = true;
        const std::vector<int32_t> no_stats;
        const std::function<void(const float*)> on_md = [&](const float* md_g) { meet->arrive(md_g, c0, c1, G); };
        if (int r = hs::cv_run_range(cv_ops, meta, no_stats, c0, c1, call.automatic_snp_threshold, per, &cv, resident, &on_md)) return fail(r);
        if (!meet->wait_for_all(G)) { set_error("hs_pipeline_run_fused: another contig group failed"); return HS_EINVAL; }
        error_rate = meet->error_rate;
    } else {
        if (int r = hs::cv_run_range(cv_ops, meta, ((const hs::CvSelection*)p->sel->impl)->rec_stats, c0, c1, call.automatic_snp_threshold, per, &cv, resident)) return r;
    }
    HipSrOps ops;
    ops.keep = &p->sr_dev_keep[(size_t)g];
    if (!via_host) ops.adopt_columns(cv_ops);
    if (int r = hs::sr_run_from_cv(ops, meta, c0, c1, cv, error_rate, call.rarest_strain_abundance, call.low_memory, call.amplicon, call.seed, per, call.window_size,
                                   &call.parts[(size_t)g], &call.sparse[(size_t)g], &p->sr_keep[(size_t)g])) return fail(r);
    if (p->recruit || p->alleles) {      // (the cells are formed on the device either way; the merge keeps the allele shares only under HS_PIPELINE_ALLELES)
        if (int r = pipeline_group_tables(call.parts[(size_t)g], call.sparse[(size_t)g], cv, call.rarest_strain_abundance, c0, ops, p->recruit ? &p->recruit_params : nullptr,
                                          call.tables[(size_t)g])) return fail(r);
    }
    // HS_PIPELINE_KEEP_COLUMNS: the entries came down beside stage 4. The two-call form copies them; the fused call's result points into
    // the group's pinned block, which stays with the pipeline until its next call
    const bool borrow = meet != nullptr;
    if (int r = hs::cv_attach_entries(cv_ops, cv, per, borrow)) return fail(r);
    if (borrow && cv && cv->entries_borrowed) p->entry_blocks[(size_t)g]->take(cv_ops.h_pk);
    return HS_OK;
}

int hs_pipeline_run(hs_pipeline* p, float automatic_snp_threshold, float error_rate, float rarest_strain_abundance, int32_t low_memory,
                    int32_t amplicon, uint32_t seed, int32_t n_threads, int32_t window_size, hs_sr_result** out, hs_pipeline_stats* st) {
    if (!p || !out || !p->sel) { set_error("hs_pipeline_run: run hs_pipeline_select first"); return HS_EINVAL; }
    if (int rc = bind_device(p->batch->device)) return rc;
    GroupCall call = group_call(p, automatic_snp_threshold, error_rate, rarest_strain_abundance, low_memory, amplicon, seed, n_threads, window_size, nullptr);
    hs::set_trace_origin();
    p->k2_order.reset();
    const int rc = p->run([&](int g) { return pipeline_group_step(p, call, g); });
    if (rc) { for (hs_sr_result* r : call.parts) if (r) hs::free_sr_result(r); return rc; }
    if (int rc_a = pipeline_merge_alleles(p, call)) { for (hs_sr_result* r : call.parts) if (r) hs::free_sr_result(r); return rc_a; }
    if (st) fold_cv_stats(st, p);      // (on top of what hs_pipeline_select wrote)
    if (std::getenv("HS_TIMING")) std::fprintf(stderr, "[hs timing] host waits so far: %ld, %.1f ms in them\n", g_waits.load(), g_wait_us.load() / 1e3);
    *out = concat_sr_parts(p, call.parts, call.sparse, st);      // (the groups' stage-3 results stay until the next call: hs_pipeline_group_cv)
    return HS_OK;
}

// hs_pipeline_select + the error rate + hs_pipeline_run in ONE call for a job that lives in one process: every contig group brings
// up its own share of the pileup (one group at a time on the device), so its host work starts a quarter of a millisecond into the
// step instead of after the pileup of the whole batch; the job-wide error rate (hs_job_rules.h: job_error_rate, then what
// hairsplitter.py makes of the printed value) is formed when the last group has its counters (GroupMeeting). mean_distance
// [n_contigs] and error_rate_out (optional) receive what hs_pipeline_select would have returned / what the caller would have computed.
int hs_pipeline_run_fused(hs_pipeline* p, float automatic_snp_threshold, float rarest_strain_abundance, int32_t low_memory, int32_t amplicon, uint32_t seed,
                          int32_t n_threads, int32_t window_size, float* mean_distance, float* error_rate_out, hs_sr_result** out, hs_pipeline_stats* st) {
    if (!p || !out) { set_error("hs_pipeline_run_fused: null argument"); return HS_EINVAL; }
    if (int rc = bind_device(p->batch->device)) return rc;
    timing_next_step();
    const int C = p->batch->n_contigs;
    static const bool timing_abs = std::getenv("HS_TIMING") != nullptr && std::string(std::getenv("HS_TIMING")) == "abs";
    const double t_enter = timing_abs ? hs::trace_ms() : 0;      // (relative to the previous call's origin: the time between two calls)
    p->drop_cv();
    p->sel = (hs_cv_selection*)std::calloc(1, sizeof(hs_cv_selection));      // (an empty selection: a two-call run may follow only after its own select)
    p->sel->impl = new hs::CvSelection();
    GroupMeeting meet;
    meet.md.assign((size_t)C, 0.f);
    GroupCall call = group_call(p, automatic_snp_threshold, 0.f, rarest_strain_abundance, low_memory, amplicon, seed, n_threads, window_size, &meet);
    hs::set_trace_origin();
    p->k2_order.reset();
    // a group that is gone (its job failed, or its thread never bound to the device) releases whoever waits for it at the meeting point
    { std::lock_guard<std::mutex> lk(p->mu); p->on_fail = [&meet] { meet.abort(); }; }
    const int rc = p->run([&](int g) { return pipeline_group_step(p, call, g); });
    { std::lock_guard<std::mutex> lk(p->mu); p->on_fail = nullptr; }
    if (rc) { for (hs_sr_result* r : call.parts) if (r) hs::free_sr_result(r); return rc; }
    if (int rc_a = pipeline_merge_alleles(p, call)) { for (hs_sr_result* r : call.parts) if (r) hs::free_sr_result(r); return rc_a; }
    if (mean_distance && C) std::memcpy(mean_distance, meet.md.data(), (size_t)C * sizeof(float));
    if (error_rate_out) *error_rate_out = meet.error_rate;
    if (st) { std::memset(st, 0, sizeof *st); fold_cv_stats(st, p); }      // (t_kernel_cv_ms[0] and [3], the pileup's own, stay 0: nothing times it apart from the chain)
    const double t_run = timing_abs ? hs::trace_ms() : 0;
    *out = concat_sr_parts(p, call.parts, call.sparse, st);
    { static const bool ps = std::getenv("HS_POOL_STATS") != nullptr; if (ps) std::fprintf(stderr, "[hs pools] device blocks allocated so far %ld, pinned %ld\n", g_pool_miss_dev.load(), g_pool_miss_host.load()); }
    if (timing_abs) std::fprintf(stderr, "[hs timing] fused call: entered @%.2f of the previous call's clock, groups done @%.2f, results merged @%.2f\n", t_enter, t_run, hs::trace_ms());
    return HS_OK;
}

int32_t hs_sr_window_size(const hs_sr_contig* contigs, int32_t n_contigs, int32_t amplicon) {
    return hs::sr_window_size(contigs, n_contigs, amplicon != 0);
}

