// hs_cv_backend.inc -- part of hs_capi.hip: stage 3 on the device. hs_cv_batch (a job's inputs resident in HBM with the launch plans)
// and HipCvOps, the HIP implementation of hs::CvDeviceOps (hs_driver.h): pileup, the column pass K2 -> candidates' bit sets queued
// without host round trips, K4 + the SNP block, loop A / loop B pair tests as opt-in kernels.
// ---------------------------------------------------------------------------------------------------
// stage 3 driver
// ---------------------------------------------------------------------------------------------------
struct hs_cv_batch {
    int32_t n_contigs = 0, n_reads = 0, n_rec = 0;
    std::vector<int64_t> contig_off, pile_off;      // pile_off [NREC + 1]: prefix sums of the records' spans (the metric's unit, the contigs' depth)
    // where record r's bytes lie in `pile`: its span rounded so that the byte of contig position p sits at an address = (contig_off + p) mod 128 -- the
    // 256 bytes a record lays over a tile of K2 / K3 then are two whole 128-byte lines (packed back to back they straddled three: K2 read 1.6 x the pileup)
    std::vector<int64_t> pile_addr;                 // [NREC + 1]; pile_addr[NREC] = bytes of the whole pileup
    int64_t pile_bytes = 0;
    std::vector<int32_t> contig_rec_off, rec_pos, rec_qend, rec_contig;
    std::vector<int64_t> rec_refspan;
    std::vector<int32_t> ploidy;      // hs_cv_batch_set_ploidy
    std::vector<int32_t> h_rank_of, h_orig_of;      // [n_rec] the reads of every contig ranked by start position (what d_rank_of / d_orig_of hold)
    mutable hs::CvMeta meta;          // the host-side description the stage drivers read, built once (batch_meta)
    mutable std::once_flag meta_once;
    int64_t total_len = 0, total_pile = 0;
    int32_t n_tasks = 0, ev_per_task = 4096, max_depth = 0;
    std::vector<int32_t> rec_task_off;      // [n_rec + 1] first pileup task of every record (tasks are listed record by record)
    int32_t n_run_tasks = 0;                // k_pileup_runs: one task per pair of 64-op chunks of a record
    std::vector<int32_t> rec_runtask_off;   // [n_rec + 1]
    int device = 0;                   // the device that was current when the batch was created: every buffer below lives there
    DBuf contig_seq, d_contig_off, read_seq, read_off, rec_read, d_rec_contig, d_rec_pos, rec_strand, rec_cig_off, cigar,
        d_pile_off, d_contig_rec_off, d_rec_qend, pile, rec_stats, rec_chunk_off, chunk_scratch,
        tile_off, tile_ent, tile_lrec, d_rank_of, d_orig_of, d_read_end, d_rank_end, run_tasks /* hsdev::RunTask per task of k_pileup_runs */, run_task_ops /* their ops, 64 HS_K1R_NCH per task */;
    HBuf h_stage_a;   // pinned staging of the per-record counters
    // what the polishing calls read of the records on the host (strand, op ranges, reads; the reads' ranges): the batch keeps them on the device,
    // the first polishing call fetches them in one shipment (polish_host_recs) and later calls find them here
    mutable std::mutex polish_mu;
    mutable bool polish_have = false;
    mutable std::vector<uint8_t> h_rec_strand;
    mutable std::vector<int64_t> h_rec_cig_off, h_read_off;
    mutable std::vector<int32_t> h_rec_read;
    // the pileup is padded by 256 bytes on both sides: k_gather_tiles loads the 256 bytes a record lays over a tile whole, also
    // where the record covers part of the tile only
    uint8_t* pile_ptr() const { return pile.as<uint8_t>() + 256; }
    // contig and read bases carry HS_SEQ_PAD readable bytes on both sides (k_pileup_runs loads whole dwords around a piece of events)
    const uint8_t* contig_ptr() const { return contig_seq.as<uint8_t>() + HS_SEQ_PAD; }
    const uint8_t* read_ptr() const { return read_seq.as<uint8_t>() + HS_SEQ_PAD; }
};

// The stage drivers allocate and free multi-megabyte arrays on many threads every call; with glibc's defaults those go
// through mmap/munmap and heap trimming, i.e. page faults and TLB shootdowns across all threads (20-ms stalls every few
// steps). Keep the memory in the process instead.
static void tune_allocator() {
    static std::once_flag once;
    std::call_once(once, [] {
        const int a = mallopt(M_MMAP_THRESHOLD, 32 << 20);      // the largest value glibc accepts
        const int b = mallopt(M_TRIM_THRESHOLD, 0x7fffffff);      // (never give freed memory back: the next call takes it again)
        const int c = mallopt(M_TOP_PAD, 64 << 20);
        if (std::getenv("HS_TIMING")) std::fprintf(stderr, "[hs timing] mallopt: mmap_threshold %d trim_threshold %d top_pad %d\n", a, b, c);
    });
}

int hs_cv_batch_create(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs,
                       const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads,
                       const int32_t* h_rec_read, const int32_t* h_rec_pos, const uint8_t* h_rec_strand,
                       const int64_t* h_rec_cig_off, const uint32_t* h_cigar, const int32_t* h_contig_rec_off,
                       hs_cv_batch** out) {
    if (int rc = require_device()) return rc;
    if (!out || n_contigs < 0) { set_error("hs_cv_batch_create: bad arguments"); return HS_EINVAL; }
    tune_allocator();
    const bool lap_on = std::getenv("HS_TIMING") != nullptr;      // (where a cold batch spends its time: spans / depth, sequences up, records up, ops up, tile plan, pileup plan, task records)
    auto lap_now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double lap_t = lap_now();
    std::string lap_s;
    auto lap = [&](const char* what) { if (!lap_on) return; const double t = lap_now(); char buf[96]; std::snprintf(buf, sizeof buf, " %s %.1f", what, t - lap_t); lap_s += buf; lap_t = t; };
    hs_cv_batch* b = new hs_cv_batch();
    HS_HIP(hipGetDevice(&b->device));
    b->n_contigs = n_contigs; b->n_reads = n_reads;
    b->contig_off.assign(h_contig_off, h_contig_off + n_contigs + 1);
    b->contig_rec_off.assign(h_contig_rec_off, h_contig_rec_off + n_contigs + 1);
    b->n_rec = b->contig_rec_off[(size_t)n_contigs];
    b->total_len = b->contig_off[(size_t)n_contigs];
    const int n_rec = b->n_rec;
    b->rec_pos.assign(h_rec_pos, h_rec_pos + n_rec);
    b->rec_contig.resize((size_t)n_rec);
    b->rec_qend.resize((size_t)n_rec);
    b->rec_refspan.resize((size_t)n_rec);
    b->pile_off.assign((size_t)n_rec + 1, 0);
    std::vector<int64_t> readspan_of((size_t)n_rec);
    {   // reference / read span of every record: one pass over all CIGAR ops, blocks of records on the host threads
        const int nb = std::max(1, std::min(n_rec / 256 + 1, 256));
        hs::hs_parallel_for(nb, host_threads(), [&](int blk) {
            const int r0 = (int)((int64_t)n_rec * blk / nb), r1 = (int)((int64_t)n_rec * (blk + 1) / nb);
            for (int r = r0; r < r1; ++r) {
                int64_t refspan = 0, readspan = 0;
                for (int64_t o = h_rec_cig_off[r]; o < h_rec_cig_off[r + 1]; ++o) {
                    const uint32_t op = h_cigar[o] & 15u; const int64_t len = h_cigar[o] >> 4;
                    if (op == 0 || op == 2 || op == 7 || op == 8) refspan += len;
                    if (op == 0 || op == 1 || op == 4 || op == 5 || op == 7 || op == 8) readspan += len;
                }
                b->rec_refspan[(size_t)r] = refspan; readspan_of[(size_t)r] = readspan;
            }
        });
    }
    for (int c = 0; c < n_contigs; ++c) {
        const int64_t L = b->contig_off[(size_t)c + 1] - b->contig_off[(size_t)c];
        for (int r = b->contig_rec_off[(size_t)c]; r < b->contig_rec_off[(size_t)c + 1]; ++r) {
            b->rec_contig[(size_t)r] = c;
            const int64_t refspan = b->rec_refspan[(size_t)r], readspan = readspan_of[(size_t)r];
            const int64_t rl = h_read_off[h_rec_read[r] + 1] - h_read_off[h_rec_read[r]];
            const int64_t pos = h_rec_pos[r];
            if (pos < 0) { set_error("negative alignment start"); delete b; return HS_EINVAL; }
            int64_t qend = pos >= L ? pos : std::min(pos + refspan, L);
            // a CIGAR that runs past the read is only tolerated for the part that lies beyond the contig end
            if (readspan > rl && pos + refspan <= L) { set_error("CIGAR consumes more bases than the read has"); delete b; return HS_EINVAL; }
            b->rec_qend[(size_t)r] = (int32_t)qend;
            b->pile_off[(size_t)r + 1] = b->pile_off[(size_t)r] + (qend - pos);
        }
    }
    b->total_pile = b->pile_off[(size_t)n_rec];
    {
        static const bool packed = std::getenv("HS_PILE_PACKED") != nullptr;      // (A/B switch: the records' bytes back to back, as before round 6)
        b->pile_addr.assign((size_t)n_rec + 1, 0);
        int64_t at = 0;
        for (int c = 0; c < n_contigs; ++c)
            for (int r = b->contig_rec_off[(size_t)c]; r < b->contig_rec_off[(size_t)c + 1]; ++r) {
                if (!packed) { const int64_t want = (b->contig_off[(size_t)c] + b->rec_pos[(size_t)r]) & 127; at += (want - at) & 127; }
                b->pile_addr[(size_t)r] = at;
                at += b->pile_off[(size_t)r + 1] - b->pile_off[(size_t)r];
            }
        b->pile_addr[(size_t)n_rec] = at;
        b->pile_bytes = at;
    }
    {   // deepest position of the batch (sweep over record starts / ends): picks the histogram counter width of K2
        std::atomic<int> deepest{0};
        hs::hs_parallel_for(n_contigs, host_threads(), [&](int c) {
            std::vector<std::pair<int32_t, int32_t>> ev;
            for (int r = b->contig_rec_off[(size_t)c]; r < b->contig_rec_off[(size_t)c + 1]; ++r)
                if (b->rec_qend[(size_t)r] > b->rec_pos[(size_t)r]) { ev.push_back(std::make_pair(b->rec_pos[(size_t)r], 1)); ev.push_back(std::make_pair(b->rec_qend[(size_t)r], -1)); }
            std::sort(ev.begin(), ev.end());
            int d = 0, dm = 0;
            for (auto& e : ev) { d += e.second; dm = std::max(dm, d); }
            int cur = deepest.load(std::memory_order_relaxed);
            while (dm > cur && !deepest.compare_exchange_weak(cur, dm, std::memory_order_relaxed)) {}
        });
        b->max_depth = std::max(b->max_depth, deepest.load());
        // what the kernels need is a bound on the depth of ONE position (K2 counts in 16-bit lanes; the reference's own loop
        // over a column's reads is a `short`, call_variants.cpp:479); the number of records on a contig is unbounded
        if (b->max_depth > 65535) { set_error("a position is covered by more than 65535 alignment records"); delete b; return HS_EINVAL; }
    }
    lap("spans+depth");
    int rc = 0;
    // (every array below goes up by the runtime's one route, upload_pageable; the first failure stops the rest)
    auto up = [&](DBuf& d, const void* src, size_t bytes, size_t pad = 0) { if (!rc) rc = upload_pageable(d, src, bytes, pad, pad); };
    up(b->contig_seq, h_contig_seq, (size_t)b->total_len, HS_SEQ_PAD);
    up(b->d_contig_off, b->contig_off.data(), sizeof(int64_t) * b->contig_off.size());
    up(b->read_seq, h_read_seq, (size_t)h_read_off[n_reads], HS_SEQ_PAD);
    up(b->read_off, h_read_off, sizeof(int64_t) * ((size_t)n_reads + 1));
    lap("sequences up");
    up(b->rec_read, h_rec_read, sizeof(int32_t) * (size_t)n_rec);
    up(b->d_rec_contig, b->rec_contig.data(), sizeof(int32_t) * (size_t)n_rec);
    up(b->d_rec_pos, h_rec_pos, sizeof(int32_t) * (size_t)n_rec);
    up(b->rec_strand, h_rec_strand, (size_t)n_rec);
    up(b->rec_cig_off, h_rec_cig_off, sizeof(int64_t) * ((size_t)n_rec + 1));
    lap("records up");
    up(b->cigar, h_cigar, sizeof(uint32_t) * (size_t)h_rec_cig_off[n_rec]);
    lap("ops up");
    up(b->d_pile_off, b->pile_addr.data(), sizeof(int64_t) * b->pile_addr.size());      // (the kernels only ask where a record's bytes begin)
    {   // tile plan of K2 / K3
        std::vector<int64_t> to; std::vector<hs_tile_entry> en; std::vector<int32_t> rc_;
        build_tile_plan(b->contig_off.data(), n_contigs, b->contig_rec_off.data(), b->rec_pos.data(), b->rec_qend.data(), b->pile_addr.data(), to, en, rc_);
        up(b->tile_off, to.data(), sizeof(int64_t) * to.size());
        up(b->tile_ent, en.data(), sizeof(hs_tile_entry) * en.size());
        for (size_t k = 0; k < rc_.size(); ++k) rc_[k] -= b->contig_rec_off[(size_t)b->rec_contig[(size_t)rc_[k]]];      // the read's index on its contig: what a column lists
        up(b->tile_lrec, rc_.data(), sizeof(int32_t) * rc_.size());
    }
    up(b->d_contig_rec_off, b->contig_rec_off.data(), sizeof(int32_t) * b->contig_rec_off.size());
    {   // what loop A on the device (k_loop_a) needs of the reads: their rank by start position on the contig (ties by index: the
        // bit order of the partition bit sets, as rank_reads() of the host glue), the inverse, the end of their alignment
        std::vector<int32_t> rec_end((size_t)n_rec), rank_of, orig_of, read_end, rank_end;
        for (int r = 0; r < n_rec; ++r) rec_end[(size_t)r] = (int32_t)std::min<int64_t>((int64_t)h_rec_pos[r] + b->rec_refspan[(size_t)r], 0x7fffffff);
        loop_a_rank_reads(b->contig_rec_off.data(), n_contigs, h_rec_pos, rec_end.data(), rank_of, orig_of, read_end, rank_end);
        up(b->d_rank_of, rank_of.data(), sizeof(int32_t) * (size_t)n_rec);
        up(b->d_orig_of, orig_of.data(), sizeof(int32_t) * (size_t)n_rec);
        b->h_rank_of = rank_of; b->h_orig_of = orig_of;
        up(b->d_read_end, read_end.data(), sizeof(int32_t) * (size_t)n_rec);
        up(b->d_rank_end, rank_end.data(), sizeof(int32_t) * 2 * (size_t)n_rec);      // (k_cand_bits: one gather per column entry)
    }
    up(b->d_rec_qend, b->rec_qend.data(), sizeof(int32_t) * (size_t)n_rec);
    lap("tile plan + ranks");
    if (!rc) {   // launch plan of the pileup kernel
        std::vector<int64_t> chunk_off((size_t)n_rec + 1);
        int32_t* tr = nullptr; int32_t* te = nullptr;
        rc = hs_pileup_plan(h_rec_cig_off, h_cigar, n_rec, b->ev_per_task, chunk_off.data(), &b->n_tasks, &tr, &te);
        if (!rc) {
            up(b->rec_chunk_off, chunk_off.data(), sizeof(int64_t) * chunk_off.size());
            b->rec_task_off.assign((size_t)n_rec + 1, 0);
            for (int32_t t = 0; t < b->n_tasks; ++t) b->rec_task_off[(size_t)tr[t] + 1]++;
            for (int r = 0; r < n_rec; ++r) b->rec_task_off[(size_t)r + 1] += b->rec_task_off[(size_t)r];
            if (!rc) rc = b->chunk_scratch.alloc(sizeof(int32_t) * 4 * (size_t)chunk_off[(size_t)n_rec]);
            {
                std::vector<int32_t> rr, rk;
                build_run_tasks(chunk_off.data(), n_rec, rr, rk, &b->rec_runtask_off);
                b->n_run_tasks = (int32_t)rr.size();
                DBuf d_rr, d_rk;      // (record, first chunk) per task: turned into the kernel's records on the device, then dropped
                up(d_rr, rr.data(), sizeof(int32_t) * rr.size());
                up(d_rk, rk.data(), sizeof(int32_t) * rk.size());
                if (!rc) rc = b->run_tasks.alloc(std::max<size_t>(1, rr.size()) * HS_RUN_TASK_BYTES);
                if (!rc) rc = b->run_task_ops.alloc(std::max<size_t>(1, rr.size()) * HS_RUN_TASK_OPS_BYTES);
                if (!rc) rc = run_task_records(d_rr.as<int32_t>(), d_rk.as<int32_t>(), b->n_run_tasks, b->d_contig_off.as<int64_t>(), b->read_off.as<int64_t>(), b->rec_read.as<int32_t>(),
                                               b->d_rec_contig.as<int32_t>(), b->d_rec_pos.as<int32_t>(), b->rec_strand.as<uint8_t>(), b->rec_cig_off.as<int64_t>(),
                                               b->d_pile_off.as<int64_t>(), b->rec_chunk_off.as<int64_t>(), b->run_tasks.p, nullptr, b->cigar.as<uint32_t>(), b->run_task_ops.as<uint32_t>());
                if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) { set_error("hs_cv_batch_create: the task records of the pileup kernel"); rc = HS_EHIP; }
            }
        }
        std::free(tr); std::free(te);
    }
    if (!rc) rc = b->pile.alloc((size_t)b->pile_bytes + 512);
    if (!rc) rc = b->rec_stats.alloc(sizeof(int32_t) * 4 * (size_t)n_rec);
    if (rc) { delete b; return rc; }
    lap("pileup plan + tasks + buffers");
    if (lap_on) std::fprintf(stderr, "[hs timing] hs_cv_batch_create laps (ms):%s\n", lap_s.c_str());
    *out = b;
    return HS_OK;
}

void hs_cv_batch_destroy(hs_cv_batch* b) { delete b; }
int64_t hs_cv_batch_aligned_bp(const hs_cv_batch* b) { return b ? b->total_pile : 0; }

void hs_cv_result_destroy(hs_cv_result* r) { hs::free_cv_result(r); }
void hs_sr_result_destroy(hs_sr_result* r) { hs::free_sr_result(r); }

}  // extern "C"

namespace {

// HIP implementation of the stage-3 device interface (the only one the product has). The columns of a contig range live in
// this object from extract_candidates() to finish_columns(); the SNP columns it leaves (snp_*) are what stage 4 reads.
struct HipCvOps : hs::CvDeviceOps, LoopADevice {
    hs_cv_batch* b;
    hipStream_t stream = nullptr;
    hipStream_t stream_late = nullptr;      // (optional) the stream of everything behind the candidates' wait: finish_columns switches to it
    explicit HipCvOps(hs_cv_batch* batch) : b(batch) {}
    KernelClock kc;

    // K1 for the records [r0, r0 + nr) of the batch on `stream` (whichever form is selected: pileup_launch), the records K0 flagged included
    int launch_k1(int r0, int nr) {
        if (nr <= 0) return HS_OK;
        if ((int)b->rec_task_off.size() != b->n_rec + 1 || (int)b->rec_runtask_off.size() != b->n_rec + 1) { set_error("launch_k1: the batch has no task index"); return HS_EINVAL; }
        const int u0 = b->rec_runtask_off[(size_t)r0], u1 = b->rec_runtask_off[(size_t)r0 + nr];
        return pileup_launch(b->contig_ptr(), b->d_contig_off.as<int64_t>(), b->read_ptr(), b->read_off.as<int64_t>(),
                             b->rec_read.as<int32_t>(), b->d_rec_contig.as<int32_t>(), b->d_rec_pos.as<int32_t>(), b->rec_strand.as<uint8_t>(),
                             b->rec_cig_off.as<int64_t>(), b->cigar.as<uint32_t>(), b->d_pile_off.as<int64_t>(),
                             b->rec_chunk_off.as<int64_t>(), b->chunk_scratch.as<int32_t>(), b->ev_per_task, b->pile_ptr(), b->rec_stats.as<int32_t>(), r0, nr, stream,
                             static_cast<const char*>(b->run_tasks.p) + (size_t)u0 * HS_RUN_TASK_BYTES, u1 - u0,
                             reinterpret_cast<const uint32_t*>(static_cast<const char*>(b->run_task_ops.p) + (size_t)u0 * HS_RUN_TASK_OPS_BYTES));
    }

    // ---- K0 + K1 over the whole batch ----
    int pileup(std::vector<int32_t>& rec_stats, float k_ms[4]) override {
        EventPair e0, e1;
        if (int rc = e0.init()) return rc;
        if (int rc = e1.init()) return rc;
        HS_HIP(ev_rec(e0.a, stream));
        if (int rc = kc.begin(HS_K_CIGAR_SCAN, stream)) return rc;
        if (int rc = cigar_scan_launch(b->d_contig_off.as<int64_t>(), b->d_rec_contig.as<int32_t>(), b->d_rec_pos.as<int32_t>(),
                                       b->rec_cig_off.as<int64_t>(), b->cigar.as<uint32_t>(), b->rec_chunk_off.as<int64_t>(), b->n_rec,
                                       b->chunk_scratch.as<int32_t>(), b->rec_stats.as<int32_t>(), stream)) return rc;
        if (int rc = kc.end((int64_t)b->cigar.bytes + (int64_t)b->chunk_scratch.bytes + 16 * (int64_t)b->n_rec, stream)) return rc;   // ops in, chunk table + counters out
        HS_HIP(ev_rec(e0.b, stream));
        HS_HIP(ev_rec(e1.a, stream));
        if (int rc = kc.begin(HS_K_PILEUP, stream)) return rc;
        if (int rc = launch_k1(0, b->n_rec)) return rc;
        if (int rc = kc.end(2 * b->total_pile, stream)) return rc;      // one read base in + one code out per aligned bp
        HS_HIP(ev_rec(e1.b, stream));
        auto grow = [](HBuf& h, size_t need) -> int { if (h.cap >= need && h.p) return HS_OK; return h.alloc(need + need / 4); };
        if (!rec_stats.empty()) {
            if (int rc = grow(b->h_stage_a, rec_stats.size() * sizeof(int32_t))) return rc;
            HS_HIP(HS_COPY_ASYNC(b->h_stage_a.p, b->rec_stats.p, rec_stats.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        }
        if (int rc = stream_wait(stream)) return rc;
        if (!rec_stats.empty()) std::memcpy(rec_stats.data(), b->h_stage_a.p, rec_stats.size() * sizeof(int32_t));
        if (int rc = e1.ms(&k_ms[0])) return rc;
        if (int rc = e0.ms(&k_ms[3])) return rc;
        kc.flush();
        return HS_OK;
    }

    // K0 + K1 of the contigs [c0, c1) queued on the stream, nothing waited for, and the contigs' mean distances formed on the device
    // (k_contig_error: call_variants.cpp:434 from K1's integer counters, and the read minimum of :463-466 that follows from it) into the
    // info block / d_min_reads: the fused pipeline's column pass starts from its own share of the pileup without the host in between
    bool own_pileup = false;
    // which = 1: K0 (the CIGAR scan: light, needs nothing of the other groups' order), 2: K1 + the records K0 flagged + the contigs' distances, 3: both
    int pileup_range_launch(int c0, int c1, float* d_mean_distance, int32_t* d_min_reads_out, int which = 3) {
        const int r0 = b->contig_rec_off[(size_t)c0], r1 = b->contig_rec_off[(size_t)c1];
        const int nr = r1 - r0;
        if ((int)b->rec_task_off.size() != b->n_rec + 1) { set_error("pileup_range: the batch has no task index"); return HS_EINVAL; }
        if (nr > 0 && (which & 1)) {
            if (int rc = kc.begin(HS_K_CIGAR_SCAN, stream)) return rc;
            if (int rc = cigar_scan_launch(b->d_contig_off.as<int64_t>(), b->d_rec_contig.as<int32_t>() + r0, b->d_rec_pos.as<int32_t>() + r0,
                                           b->rec_cig_off.as<int64_t>() + r0, b->cigar.as<uint32_t>(), b->rec_chunk_off.as<int64_t>() + r0, nr,
                                           b->chunk_scratch.as<int32_t>(), b->rec_stats.as<int32_t>() + 4 * (size_t)r0, stream)) return rc;
            const double share = b->n_rec > 0 ? (double)nr / (double)b->n_rec : 0.0;
            if (int rc = kc.end((int64_t)(share * ((double)b->cigar.bytes + (double)b->chunk_scratch.bytes)) + 16 * (int64_t)nr, stream)) return rc;
        }
        if (!(which & 2)) return HS_OK;
        if (nr > 0) {
            const int t0 = b->rec_task_off[(size_t)r0], t1 = b->rec_task_off[(size_t)r1];
            if (int rc = kc.begin(HS_K_PILEUP, stream)) return rc;
            int64_t range_pile = 0;
            if (t1 > t0) {
                if (int rc = launch_k1(r0, nr)) return rc;
                range_pile = b->pile_off[(size_t)r1] - b->pile_off[(size_t)r0];
            }
            if (int rc = kc.end(2 * range_pile, stream)) return rc;      // one read base in + one code out per aligned bp
        }
        hipLaunchKernelGGL(hsdev::k_contig_error, dim3((unsigned)((c1 - c0 + 3) / 4)), dim3(256), 0, stream, b->rec_stats.as<int32_t>(), b->d_contig_rec_off.as<int32_t>(), c0, c1 - c0,
                           d_mean_distance, d_min_reads_out);
        HS_HIP(hipGetLastError());
        return HS_OK;
    }
    static int h_info_grow(HBuf& h, size_t need) { if (h.cap >= need && h.p) return HS_OK; return h.alloc(need + need / 4); }

    // ---- the columns of the current contig range ----
    int range_c0 = 0, range_c1 = 0;
    int64_t n_cols = 0, n_entries = 0;            // extracted columns / their entries
    SelectionScratch range_scratch;               // K2's per-tile slots
    DBuf d_tile_ent_sum, d_tile_ebase, d_scan2, d_sel_info;
    DBuf d_col_gpos, d_col_rec, d_co, d_col_len, d_ci, d_cc;      // d_co / d_ci / d_cc: the CSR of the columns (also read by k_loop_a_prepare)
    DBuf d_col_ctg, d_k0, d_k1, d_c1, d_cand, d_ctg_col_off, d_min_reads, d_blk_cnt, d_blk_ent;
    // what the host reads between the phases, one small block = one download: [ColumnsHeader 64 B][tie counters 4 x 16 B][per-contig counts 4 C]
    DBuf d_info; HBuf h_info;
    hsdev::ColumnsHeader* dev_header() const { return d_info.as<hsdev::ColumnsHeader>(); }
    unsigned long long* dev_tie() const { return (unsigned long long*)((char*)d_info.p + 64); }
    // behind the two counters: per contig of the range the candidates [C], the SNPs [C] and the SNP bounds [2 C], cleared with the header
    int32_t* dev_ctg_n() const { return (int32_t*)((char*)d_info.p + 128); }
    int32_t* dev_ctg_snp() const { return dev_ctg_n() + (range_c1 - range_c0); }
    int32_t* dev_snp_bounds() const { return dev_ctg_n() + 2 * (range_c1 - range_c0); }
    const hsdev::ColumnsHeader& host_header() const { return *(const hsdev::ColumnsHeader*)h_info.p; }
    const int32_t* host_ctg_n() const { return (const int32_t*)((const char*)h_info.p + 128); }
    const int32_t* host_ctg_snp() const { return host_ctg_n() + (range_c1 - range_c0); }
    // ... and, for a range that brought up its own pileup, the contigs' mean distances [C floats]
    static size_t info_bytes(int C) { return (128 + (size_t)C * 20 + 15) & ~(size_t)15; }
    float* dev_ctg_md() const { return (float*)(dev_ctg_n() + 4 * (range_c1 - range_c0)); }
    const float* host_ctg_md() const { return (const float*)(host_ctg_n() + 4 * (range_c1 - range_c0)); }
    // the flagged columns (candidates, later the SNPs) packed into ONE block = one download: [records 16 nf][column index 4 nf][offsets 8 (nf + 1)]
    // [read indices 4 ne][codes ne], every part 256-byte aligned; the SNP block is what stage 4 takes over (HipSrOps::adopt_columns)
    DBuf d_pk; HBuf h_pk;
    struct PackLayout { size_t rec, col, off, idx, code, total, head, len; bool light; };
    static PackLayout pack_layout(int64_t nf, int64_t ne, bool light = false) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        PackLayout L;
        L.light = light;
        L.rec = 0; L.col = up((size_t)nf * 16); L.off = L.col + up((size_t)nf * 4); L.idx = L.off + up(((size_t)nf + 1) * 8);
        L.head = L.idx;
        if (light) { L.len = L.idx; L.code = L.len + up((size_t)nf * 4); L.total = L.code + 256; }      // (records, column indices, places, lengths: no entries)
        else { L.len = 0; L.code = L.idx + up((size_t)ne * 4); L.total = L.code + up((size_t)ne + 1); }
        return L;
    }
    PackLayout pk_layout{};
    UploadPack range_pack;
    int n_gathered = 0;                           // (k_loop_a_prepare checks its column indices against it)
    int64_t gathered_entries = 0;
    static int grow(HBuf& h, size_t need) { if (h.cap >= need && h.p) return HS_OK; return h.alloc(need + need / 4); }
    static int grow(DBuf& d, size_t need) { if (d.cap >= need && d.p && !d.view) { d.bytes = need; return HS_OK; } return d.alloc(need + need / 4); }

    // What a call learnt about the sizes of this contig range, kept by the caller from step to step (a pipeline group runs the same
    // contigs again and again; a service runs batches of the same shape): with it the arrays are sized ahead and the whole column
    // pass, K2 to the candidates' bit sets, is queued without a host round trip; every kernel checks the capacities it was given and
    // a pass whose numbers did not fit (the header says so) is run again the careful way, sizes first.
    struct Keep {
        bool valid = false;
        int64_t cols = 0, entries = 0, cand = 0, cand_entries = 0, cb_words = 0, snp = 0, snp_entries = 0, ties = -1;
        std::vector<int32_t> cand_per_contig;      // the candidates of every contig last time: what the split of loop A between device and host is made from
        std::vector<uint8_t> la_force_host;        // contigs the device gave up on once (its tables do not hold them): the host's from then on
        int64_t la_span = 0;                       // words of all partition spans the device's loop A left last time
        hipEvent_t k2_done = nullptr;      // K2 of the groups one after the other on the device (DeviceTurn without the host in it)
        hipStream_t side = nullptr;        // the SNP columns' entries leave on this stream, beside stage 4 (defer_entries)
        hipEvent_t packed = nullptr;
        ~Keep() { if (k2_done) (void)hipEventDestroy(k2_done); if (packed) (void)hipEventDestroy(packed); if (side) (void)hipStreamDestroy(side); }
    };
    // per pipeline: the groups queue their K2 in group order (group 0 first: the groups are cut so that the early ones are the big ones),
    // each behind the event of the one before
    struct K2Order {
        std::mutex mu; std::condition_variable cv; hipEvent_t last = nullptr; int next = 0;
        void reset() { std::lock_guard<std::mutex> lk(mu); next = 0; }
        void abort() { { std::lock_guard<std::mutex> lk(mu); next = 1 << 30; } cv.notify_all(); }      // (a group failed: nobody waits for its turn)
    };
    struct K2Turn {      // holds the order's lock from this group's turn on; passes the turn on when it goes out of scope at the latest
        K2Order* o = nullptr; std::unique_lock<std::mutex> lk; bool passed = true;
        void take(K2Order* order, int ticket) {
            o = order; lk = std::unique_lock<std::mutex>(o->mu);
            if (ticket >= 0) o->cv.wait(lk, [&] { return o->next >= ticket; });
            passed = false;
        }
        void pass() { if (!passed) { passed = true; o->next++; lk.unlock(); o->cv.notify_all(); } }
        bool held() const { return !passed; }
        ~K2Turn() { pass(); }
    };
    int order_ticket = -1;             // this group's place in the order (-1: whoever comes first)
    Keep* keep = nullptr;
    K2Order* k2_order = nullptr;
    static int64_t with_margin(int64_t v) { return v + v / 8 + 1024; }
    static bool hints_on() { static const bool off = std::getenv("HS_NO_SIZE_HINTS") != nullptr; return !off; }

    int fetch_info() {      // the info block from the device (one transfer + wait)
        const size_t bytes = info_bytes(range_c1 - range_c0);
        if (int rc = grow(h_info, bytes)) return rc;
        Shipment sh; sh.add(h_info.p, d_info.p, bytes);
        if (int rc = sh.launch(stream, 1)) return rc;
        return stream_wait(stream);
    }
    // the columns carrying `flag`: block sums + offsets (the header then holds their number and their entries) ...
    int flag_sums_launch(int flag, int64_t cols_cap) {
        const int n_blocks = (int)((cols_cap + HS_FP_BLOCK - 1) / HS_FP_BLOCK);
        if (int rc = grow(d_blk_cnt, std::max<size_t>(1, (size_t)n_blocks) * 8)) return rc;
        if (int rc = grow(d_blk_ent, std::max<size_t>(1, (size_t)n_blocks) * 8)) return rc;
        if (int rc = kc.begin(HS_K_PACK_COLUMNS, stream)) return rc;
        if (n_blocks > 0)
            hipLaunchKernelGGL(hsdev::k_flag_block_sums, dim3((unsigned)n_blocks), dim3(256), 0, stream, d_col_rec.as<hsdev::hs_colrec_dev>(), d_col_len.as<int32_t>(),
                               dev_header(), flag, d_blk_cnt.as<long long>(), d_blk_ent.as<long long>());
        hipLaunchKernelGGL(hsdev::k_flag_block_offsets, dim3(1), dim3(1024), 0, stream, d_blk_cnt.as<long long>(), d_blk_ent.as<long long>(), n_blocks, dev_header());
        HS_HIP(hipGetLastError());
        return kc.end(20 * cols_cap, stream);      // record + length of every column in
    }
    // ... and packed on the device (d_pk, laid out for the capacities cap_f columns / cap_e entries)
    int pack_launch(int flag, int64_t cols_cap, int64_t cap_f, int64_t cap_e, bool light = false) {
        const int n_blocks = (int)((cols_cap + HS_FP_BLOCK - 1) / HS_FP_BLOCK);
        pk_layout = pack_layout(cap_f, cap_e, light);
        const PackLayout& L = pk_layout;
        if (int rc = grow(d_pk, L.total)) return rc;
        char* base = (char*)d_pk.p;
        hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, reinterpret_cast<uint4*>(base + L.off), 1ll, 0u);      // (no flagged column: offsets[0] = 0)
        if (n_blocks == 0) { HS_HIP(hipGetLastError()); return HS_OK; }
        if (int rc = kc.begin(HS_K_PACK_COLUMNS, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_pack_flagged, dim3((unsigned)n_blocks), dim3(1024), 0, stream, d_col_rec.as<hsdev::hs_colrec_dev>(), d_co.as<int64_t>(),
                           d_col_len.as<int32_t>(), d_ci.as<int32_t>(), d_cc.as<uint8_t>(), dev_header(), flag, d_blk_cnt.as<long long>(),
                           d_blk_ent.as<long long>(), (hsdev::hs_colrec_dev*)(base + L.rec), (int32_t*)(base + L.col), (int64_t*)(base + L.off), (int32_t*)(base + L.idx),
                           (uint8_t*)(base + L.code), cap_f, cap_e, light ? (int32_t*)(base + L.len) : nullptr);
        HS_HIP(hipGetLastError());
        return kc.end((light ? 0 : 10 * cap_e) + 60 * cap_f, stream);      // the flagged columns' entries in and out (not in the light form), their records
    }

    // The packed candidates as bit sets (k_cand_bits) straight into pinned host memory, with their records and the info block: what
    // loop A reads. The word blocks are bump-allocated on the device (cap_words).
    DBuf d_cb_bits, d_cb_words, d_cb_counter;
    HBuf h_cb;
    struct CbLayout { size_t rec, bits, words, total; int64_t cap_cand, cap_words; } cbl{};
    int cand_bits_launch(int64_t cap_cand, int64_t cap_cand_entries, int64_t cap_words, bool skip_device_contigs = false) {
        static_assert(sizeof(hs::CandBits) == sizeof(hsdev::CandBitsDev), "CandBits layout");
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        cbl.cap_cand = cap_cand; cbl.cap_words = cap_words;
        cbl.rec = 256; cbl.bits = cbl.rec + up((size_t)cap_cand * 16); cbl.words = cbl.bits + up((size_t)cap_cand * 32); cbl.total = cbl.words + up((size_t)cap_words * 8);
        if (int rc = grow(d_cb_bits, std::max<size_t>(1, (size_t)cap_cand) * 32)) return rc;
        if (int rc = grow(d_cb_words, std::max<size_t>(1, (size_t)cap_words) * 8)) return rc;
        if (int rc = grow(d_cb_counter, 256)) return rc;
        if (int rc = grow(h_cb, cbl.total)) return rc;
        const char* cb = (const char*)d_cand_pk.p;
        hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, d_cb_counter.as<uint4>(), 16ll, 0u);
        if (cap_cand > 0) {
            if (int rc = kc.begin(HS_K_CAND_BITS, stream)) return rc;
            hipLaunchKernelGGL(hsdev::k_cand_bits, dim3((unsigned)((cap_cand + HS_CB_WAVES * HS_CB_PER_WAVE - 1) / (HS_CB_WAVES * HS_CB_PER_WAVE))), dim3(64 * HS_CB_WAVES), 0, stream,
                               (const hsdev::hs_colrec_dev*)(cb + cand_layout.rec), (const int64_t*)(cb + cand_layout.off),
                               cand_layout.light ? d_ci.as<int32_t>() : (const int32_t*)(cb + cand_layout.idx), cand_layout.light ? d_cc.as<uint8_t>() : (const uint8_t*)(cb + cand_layout.code),
                               dev_header(), (long long)cap_cand, b->d_contig_rec_off.as<int32_t>(), b->d_rank_end.as<int2>(),
                               d_cb_bits.as<hsdev::CandBitsDev>(), d_cb_words.as<unsigned long long>(), (long long)cap_words,
                               d_cb_counter.as<unsigned long long>(), (long long)cap_cand_entries, cand_layout.light ? (const int32_t*)(cb + cand_layout.len) : nullptr,
                               skip_device_contigs && la_plan.n_dev > 0 ? d_la_on.as<uint8_t>() : nullptr, range_c0);
            HS_HIP(hipGetLastError());
            if (int rc = kc.end(5 * cap_cand_entries + 48 * cap_cand, stream)) return rc;      // the candidates' entries in; record, header and block out
        }
        Shipment sh;
        sh.add(h_cb.p, d_cb_counter.p, 16);
        const long long* n_flagged = reinterpret_cast<const long long*>((const char*)d_info.p + offsetof(hsdev::ColumnsHeader, n_flagged));
        sh.add_counted((char*)h_cb.p + cbl.rec, cb + cand_layout.rec, n_flagged, 16, cap_cand);
        sh.add_counted((char*)h_cb.p + cbl.bits, d_cb_bits.p, n_flagged, 32, cap_cand);
        sh.add_counted((char*)h_cb.p + cbl.words, d_cb_words.p, d_cb_counter.as<long long>(), 8, cap_words);
        if (int rc = grow(h_info, info_bytes(range_c1 - range_c0))) return rc;
        sh.add(h_info.p, d_info.p, info_bytes(range_c1 - range_c0));
        if (int rc = kc.begin(HS_K_SHIP, stream)) return rc;
        if (int rc = sh.launch(stream)) return rc;
        return kc.end(0, stream);
    }
    // after the wait: did the capacities hold?
    bool cand_bits_fit() const { const unsigned long long* cnt = (const unsigned long long*)h_cb.p; return cnt[1] == 0; }
    int64_t cand_bits_words() const { return (int64_t)((const unsigned long long*)h_cb.p)[0]; }
    void cand_bits_result(hs::CvCandidates& out) const {
        out.rec = (const hs_colrec*)((const char*)h_cb.p + cbl.rec);
        out.bits = (const hs::CandBits*)((const char*)h_cb.p + cbl.bits);
        out.words = (const uint64_t*)((const char*)h_cb.p + cbl.words);
    }
    int fetch_candidates(hs::CvCandidates& out) override {      // the candidates of the last extract_candidates() for the host's loop A, after all
        out.bits = nullptr; out.words = nullptr;
        if (cand_count == 0) return HS_OK;
        int64_t cap_words = std::max<int64_t>(with_margin(keep ? keep->cb_words : 0), 16 * cand_count + cand_entries / 4 + 64);
        for (int attempt = 0;; ++attempt) {
            if (int rc = cand_bits_launch(cand_count, cand_entries, cap_words)) return rc;
            if (int rc = stream_wait(stream)) return rc;
            if (cand_bits_fit()) { if (keep) keep->cb_words = cand_bits_words(); cand_bits_result(out); return HS_OK; }
            if (attempt >= 4 || cand_bits_words() <= cap_words) { set_error("candidate bit sets: the blocks do not fit (a column over more than 65535 words of reads?)"); return HS_EINVAL; }
            cap_words = cand_bits_words() + 64;      // (the counter ran on past the capacity: it is the exact need)
        }
    }
    DBuf d_cand_pk;                   // the packed candidates (kept beside d_pk, which the SNPs take later): k_cand_bits and k_loop_a read them
    PackLayout cand_layout{};
    int64_t cand_count = 0, cand_entries = 0;
    std::vector<int32_t> cand_per_contig;
    int extract_candidates(int c0, int c1, const std::vector<int32_t>& min_reads, float thr, hs::CvCandidates& out, float k_ms[3], bool want_entries) override {
        const bool hinted = keep && keep->valid && want_entries && hints_on();
        if (hinted) {
            const int rc = extract_candidates_impl(c0, c1, min_reads, thr, out, k_ms, want_entries, true);
            if (rc != HS_EAGAIN_SIZES) return rc;
            keep->valid = false;      // (the sizes of this range have changed: the careful way, which also takes the new ones)
            if (int rc2 = stream_wait(stream)) return rc2;      // (what the first pass queued reads blocks the second one sizes anew)
        }
        return extract_candidates_impl(c0, c1, min_reads, thr, out, k_ms, want_entries, false);
    }
    static constexpr int HS_EAGAIN_SIZES = -1000;      // (internal: a capacity did not hold)
    int extract_candidates_impl(int c0, int c1, const std::vector<int32_t>& min_reads, float thr, hs::CvCandidates& out, float k_ms[3], bool want_entries, bool hinted) {
        static_assert(sizeof(hs_colrec) == sizeof(hsdev::hs_colrec_dev), "hs_colrec layout");
        static_assert(sizeof(hsdev::ColumnsHeader) == 64, "info block layout");
        const int C = c1 - c0;
        range_c0 = c0; range_c1 = c1; n_cols = 0; n_entries = 0; n_gathered = 0; gathered_entries = 0;
        cand_count = 0; cand_entries = 0;
        out = hs::CvCandidates();
        out.contig_n_cand.assign((size_t)C, 0);
        k_ms[0] = k_ms[1] = k_ms[2] = 0;
        const int64_t g0 = b->contig_off[(size_t)c0], g1 = b->contig_off[(size_t)c1];
        if (g1 <= g0 || C <= 0) return HS_OK;
        const int64_t t0 = g0 >> 8, t1 = (g1 + 255) >> 8, nt = t1 - t0;
        if (nt > 0x7fffffff) { set_error("too many tiles in one contig range"); return HS_EINVAL; }
        EventPair e_k2, e_k3, e_k3b;
        if (int rc = e_k2.init()) return rc;
        if (int rc = e_k3.init()) return rc;
        if (int rc = e_k3b.init()) return rc;
        const size_t info_b = info_bytes(C);
        if (int rc = grow(d_info, info_b)) return rc;
        if (own_pileup) { if (int rc = grow(d_min_reads, std::max<size_t>(1, (size_t)C) * 4)) return rc; }
        if (int rc = range_scratch.prepare(nt * 256)) return rc;
        if (int rc = grow(d_tile_ent_sum, (size_t)nt * 4)) return rc;
        if (int rc = grow(d_tile_ebase, ((size_t)nt + 1) * 8)) return rc;
        // K2 forms the leading codes of what it selects and drops the positions nobody reads
        if (int rc = grow(d_sel_info, (size_t)nt * 256 * 8)) return rc;
        bool k2_info = false;
        const int64_t range_pile = b->total_len > 0 ? (int64_t)((double)b->total_pile * (double)(g1 - g0) / (double)b->total_len) : 0;      // one code in per aligned bp of the range (its share of the batch)
        // The head of the pass in three parts: what needs no turn (the info block cleared, K0 over the group's records), the kernels that fill
        // the device on their own (K1, K2: the groups' turns, one after the other on the device), and the two scans over K2's per-tile counts
        // (small: outside the turn again -- the next group's K1 starts when this group's K2 ends, not 0.12 ms of scan launches later).
        auto k2_pre = [&]() -> int {
            hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(256), 0, stream, d_info.as<uint4>(), (long long)(info_b / 16), 0u);      // (header, tie counters, candidates / SNPs / SNP bounds per contig)
            if (own_pileup) { if (int rc = pileup_range_launch(c0, c1, dev_ctg_md(), d_min_reads.as<int32_t>(), 1)) return rc; }
            return HS_OK;
        };
        auto k2_main = [&]() -> int {   // ---- K2 over the tiles of the range: per tile its selected positions (second count >= 4), their depths and the sum of those ----
            if (own_pileup) { if (int rc = pileup_range_launch(c0, c1, dev_ctg_md(), d_min_reads.as<int32_t>(), 2)) return rc; }
            HS_HIP(ev_rec(e_k2.a, stream));
            if (int rc = kc.begin(HS_K_COLUMN_STATS, stream)) return rc;
            hipEvent_t k2_done = nullptr;
            if (int rc = kc.end_prepare(range_pile, &k2_done)) return rc;
            if (int rc = column_stats_tiled_launch(b->pile_ptr(), b->tile_off.as<int64_t>(), b->tile_ent.as<hs_tile_entry>(), b->total_len, nullptr, 4,
                                                   range_scratch.tile_cnt.as<int32_t>() /* (only "selection wanted") */, nullptr, nullptr, 0, b->max_depth, &range_scratch,
                                                   e_k2.b, stream, k2_done, t0, t1, g0, g1, d_tile_ent_sum.as<int32_t>(), false, true,
                                                   d_sel_info.as<uint2>(), &k2_info)) return rc;
            return HS_OK;
        };
        auto k2_post = [&]() -> int {
            if (int rc = exclusive_scan_launch(range_scratch.tile_cnt.as<int32_t>(), (int)nt, range_scratch.tile_base.as<int64_t>(), range_scratch.scan_scratch, stream)) return rc;
            return exclusive_scan_launch(d_tile_ent_sum.as<int32_t>(), (int)nt, d_tile_ebase.as<int64_t>(), d_scan2, stream);
        };
        auto k2_launch = [&]() -> int { if (int rc = k2_pre()) return rc; if (int rc = k2_main()) return rc; return k2_post(); };
        int64_t cap_cols = 0, cap_entries = 0;
        K2Turn order_lock;
        if (!hinted) {
            DeviceTurn turn;
            if (int rc = k2_launch()) return rc;
            // the two totals (the last elements of the scans) -> sizes of the column arrays
            hipLaunchKernelGGL(hsdev::k_columns_totals, dim3(1), dim3(64), 0, stream, range_scratch.tile_base.as<int64_t>() + nt, d_tile_ebase.as<int64_t>() + nt, dev_header());
            HS_HIP(hipGetLastError());
            if (int rc = fetch_info()) return rc;
            cap_cols = host_header().n_cols; cap_entries = host_header().n_entries;
        } else {
            // the groups' K2 launches one after the other ON THE DEVICE (each fills it on its own, see DeviceTurn): this group's
            // launch queues behind the event of the group that came before it, no host thread waits for anything
            // What queues behind the previous group: the group's share of the pileup (fused call) and its K2 -- the kernels that fill the
            // device on their own. Ordering the whole chain up to the shipment of the candidates as well was measured in round 4:
            // 19.7 ms per C4 step against 17.9 (the small kernels behind K2 overlap better across the groups than they queue).
            if (k2_order && DeviceTurn::on()) {
                if (int rc = k2_pre()) return rc;      // (before the turn: every group's K0 is on the device when the step begins)
                order_lock.take(k2_order, order_ticket);
                if (!keep->k2_done) HS_HIP(hipEventCreateWithFlags(&keep->k2_done, hipEventDisableTiming));
                if (k2_order->last && k2_order->last != keep->k2_done) HS_HIP(hipStreamWaitEvent(stream, k2_order->last, 0));
                if (int rc = k2_main()) return rc;
                HS_HIP(ev_rec(keep->k2_done, stream)); k2_order->last = keep->k2_done; order_lock.pass();
                if (int rc = k2_post()) return rc;
            } else if (int rc = k2_launch()) return rc;
            cap_cols = with_margin(keep->cols); cap_entries = with_margin(keep->entries);
        }
        if (cap_cols > 0x7fffffff) { set_error("more than 2^31 columns in one contig range"); return HS_EINVAL; }
        if (int rc = grow(d_col_gpos, std::max<size_t>(1, (size_t)cap_cols) * 8)) return rc;
        if (int rc = grow(d_col_rec, std::max<size_t>(1, (size_t)cap_cols) * sizeof(hs_colrec))) return rc;
        if (int rc = grow(d_co, ((size_t)cap_cols + 1) * 8)) return rc;
        if (int rc = grow(d_col_len, std::max<size_t>(1, (size_t)cap_cols) * 4)) return rc;
        if (int rc = grow(d_ci, std::max<size_t>(1, (size_t)cap_entries) * 4)) return rc;
        if (int rc = grow(d_cc, std::max<size_t>(1, (size_t)cap_entries))) return rc;
        if (int rc = grow(d_col_ctg, std::max<size_t>(1, (size_t)cap_cols) * 4)) return rc;
        if (int rc = grow(d_k0, std::max<size_t>(1, (size_t)cap_cols))) return rc;
        if (int rc = grow(d_k1, std::max<size_t>(1, (size_t)cap_cols))) return rc;
        if (int rc = grow(d_c1, std::max<size_t>(1, (size_t)cap_cols) * 4)) return rc;
        if (int rc = grow(d_cand, std::max<size_t>(1, (size_t)cap_cols))) return rc;
        if (int rc = grow(d_ctg_col_off, ((size_t)C + 1) * 8)) return rc;
        if (!own_pileup) { range_pack.add(min_reads, d_min_reads); if (int rc = range_pack.commit(stream)) return rc; }
        // ---- the column list with its CSR offsets, K3 (tile-cooperative gather), K3b (leading codes, reference order), V1 ----
        if (int rc = kc.begin(HS_K_COLUMNS_COMPACT, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_columns_compact, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, stream, range_scratch.tile_cnt.as<int32_t>(), range_scratch.tile_base.as<int64_t>(),
                           d_tile_ebase.as<int64_t>(), range_scratch.gpos.as<int64_t>(), range_scratch.depth.as<int32_t>(), nt, b->d_contig_off.as<int64_t>(), b->n_contigs,
                           d_col_gpos.as<int64_t>(), d_col_rec.as<hsdev::hs_colrec_dev>(), d_co.as<int64_t>(), d_col_len.as<int32_t>(), dev_header(), cap_cols, cap_entries,
                           k2_info ? d_sel_info.as<uint2>() : nullptr);
        HS_HIP(hipGetLastError());
        if (int rc = kc.end(20 * nt + 56 * cap_cols, stream)) return rc;      // tile counts and bases in; slot in, position + record + offset + length out per column
        HS_HIP(ev_rec(e_k3.a, stream));
        if (cap_cols > 0) {
            if (int rc = kc.begin(HS_K_GATHER_COLUMNS, stream)) return rc;
            // (tiles with up to HS_GT_DIRECT kept positions -- nearly all -- in the form without LDS, the others through the staged rows)
            hipLaunchKernelGGL(hsdev::k_gather_tiles_direct, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, stream, b->pile_ptr(), b->tile_off.as<int64_t>(),
                               reinterpret_cast<const int4*>(b->tile_ent.as<hs_tile_entry>()), b->tile_lrec.as<int32_t>(), t0, nt, range_scratch.tile_cnt.as<int32_t>(),
                               range_scratch.tile_base.as<int64_t>(), d_col_gpos.as<int64_t>(), d_co.as<int64_t>(), d_ci.as<int32_t>(), d_cc.as<uint8_t>(), dev_header());
            hipLaunchKernelGGL(hsdev::k_gather_tiles, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, stream, b->pile_ptr(), b->tile_off.as<int64_t>(),
                               reinterpret_cast<const int4*>(b->tile_ent.as<hs_tile_entry>()), b->tile_lrec.as<int32_t>(), t0, nt, range_scratch.tile_cnt.as<int32_t>(),
                               range_scratch.tile_base.as<int64_t>(), d_col_gpos.as<int64_t>(), d_co.as<int64_t>(), d_ci.as<int32_t>(), d_cc.as<uint8_t>(), dev_header());
            HS_HIP(hipGetLastError());
            // the pileup bytes of the range's tiles in (every one of them once), read index + code out per column entry
            if (int rc = kc.end(range_pile + 5 * (hinted ? keep->entries : cap_entries), stream)) return rc;
        }
        HS_HIP(ev_rec(e_k3.b, stream));
        HS_HIP(ev_rec(e_k3b.a, stream));
        if (cap_cols > 0) {
            if (int rc = kc.begin(HS_K_COLUMN_TOP3, stream)) return rc;
            // the columns whose leading codes K2 left open (equal counts; all of them without K2's second pass): a wavefront per 64 records
            const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((cap_cols + 4 * HS_T3_CHUNK - 1) / (4 * HS_T3_CHUNK), 65536));
            hipLaunchKernelGGL(hsdev::k_column_top3_exact, dim3(grid), dim3(256), 0, stream, d_co.as<int64_t>(), d_col_len.as<int32_t>(), d_cc.as<uint8_t>(),
                               dev_header(), d_col_rec.as<hsdev::hs_colrec_dev>(), dev_tie());
            HS_HIP(hipGetLastError());
            const int64_t cols_now = hinted ? keep->cols : cap_cols, ents_now = hinted ? keep->entries : cap_entries;
            const int64_t n_und = k2_info ? (keep && keep->ties >= 0 ? keep->ties : cols_now / 32) : cols_now;
            const int64_t avg = cols_now > 0 ? ents_now / cols_now : 0;
            if (int rc = kc.end(16 * cols_now + n_und * (avg + 28), stream)) return rc;      // (every record in; the open columns' codes, offset and length in, the record out)
        }
        if (int rc = kc.begin(HS_K_CANDIDATES_SCAN, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_candidates_scan, dim3((unsigned)((std::max<int64_t>(cap_cols, C) + 255) / 256)), dim3(256), 0, stream, d_col_gpos.as<int64_t>(), dev_header(),
                           b->d_contig_off.as<int64_t>(), c0, C, d_min_reads.as<int32_t>(), thr, d_col_rec.as<hsdev::hs_colrec_dev>(), d_col_ctg.as<int32_t>(),
                           d_k0.as<uint8_t>(), d_k1.as<uint8_t>(), d_c1.as<int32_t>(), d_cand.as<uint8_t>(), d_ctg_col_off.as<int64_t>(), dev_ctg_n());
        HS_HIP(hipGetLastError());
        if (int rc = kc.end(43 * (hinted ? keep->cols : cap_cols), stream)) return rc;      // record in and out, the four arrays K4 reads out
        HS_HIP(ev_rec(e_k3b.b, stream));
        // ---- the candidates, packed (they stay on the device); the host's loop A gets them as bit sets ----
        if (int rc = flag_sums_launch(HS_COL_CAND, cap_cols)) return rc;
        int64_t cap_cand = 0, cap_cand_entries = 0, cap_words = 0;
        if (!hinted) {
            if (int rc = fetch_info()) return rc;      // (carries the per-contig counts and the tie counters too)
            cap_cand = host_header().n_flagged; cap_cand_entries = host_header().n_flagged_entries;
            cap_words = std::max<int64_t>(with_margin(keep ? keep->cb_words : 0), 16 * cap_cand + cap_cand_entries / 4 + 64);
        } else { cap_cand = with_margin(keep->cand); cap_cand_entries = with_margin(keep->cand_entries); cap_words = with_margin(keep->cb_words); }
        // (the host's loop A reads bit sets: k_cand_bits takes the candidates' entries where the gather left them, nothing is copied; the
        // device's loop A reads the packed entries)
        if (int rc = pack_launch(HS_COL_CAND, cap_cols, cap_cand, cap_cand_entries, want_entries)) return rc;
        cand_layout = pk_layout;
        std::swap(d_cand_pk, d_pk);      // (d_pk is packed again for the SNPs)
        if (want_entries) {
            // loop A of the contigs that fit the device's tables runs there (k_loop_a), queued behind the bit sets of the others: the host
            // waits for those only (an event in the middle of the stream) and walks its share while the device walks its own
            la_launched = false;
            la_plan = LoopADevice::LoopAPlan();
            if (loop_a_device_max() > 0) {
                const bool counts_known = hinted ? (int)keep->cand_per_contig.size() == C : true;      // (not hinted: the info block has just been read)
                if (counts_known) { if (int rc = loop_a_plan(hinted ? keep->cand_per_contig.data() : host_ctg_n(), C)) return rc; }
            }
            for (int attempt = 0;; ++attempt) {
                if (int rc = cand_bits_launch(cap_cand, cap_cand_entries, cap_words, true)) return rc;
                if (order_lock.held()) { HS_HIP(ev_rec(keep->k2_done, stream)); k2_order->last = keep->k2_done; order_lock.pass(); }
                if (la_plan.n_dev > 0 && attempt == 0) {
                    if (!ev_cand) { if (int rc = EventPair::get(&ev_cand)) return rc; }
                    HS_HIP(hipEventRecord(ev_cand, stream));
                    if (int rc = loop_a_launch(cap_cand)) return rc;
                    if (int rc = event_wait(ev_cand)) return rc;
                } else if (int rc = stream_wait(stream)) return rc;
                if (cand_bits_fit()) break;
                if (hinted) return HS_EAGAIN_SIZES;
                if (attempt >= 4 || cand_bits_words() <= cap_words) { set_error("candidate bit sets: the blocks do not fit (a column over more than 65535 words of reads?)"); return HS_EINVAL; }
                cap_words = cand_bits_words() + 64;      // (the counter ran on past the capacity: it is the exact need)
            }
        } else if (int rc = fetch_info()) return rc;
        const hsdev::ColumnsHeader& H = host_header();
        if (hinted && (!H.ok || H.n_cols > cap_cols || H.n_entries > cap_entries || H.n_flagged > cap_cand || H.n_flagged_entries > cap_cand_entries)) return HS_EAGAIN_SIZES;
        n_cols = H.n_cols; n_entries = H.n_entries;
        out.n_columns = n_cols; out.n_entries = n_entries;
        n_gathered = (int)n_cols; gathered_entries = n_entries;
        std::memcpy(out.contig_n_cand.data(), host_ctg_n(), (size_t)C * 4);
        if (own_pileup) out.contig_mean_distance.assign(host_ctg_md(), host_ctg_md() + C);
        cand_per_contig = out.contig_n_cand; cand_count = H.n_flagged; cand_entries = H.n_flagged_entries;
        if (la_launched) out.contig_on_device = la_plan.on_dev;
        { unsigned long long t8[8]; std::memcpy(t8, (const char*)h_info.p + 64, 64); out.n_tie = (int64_t)(t8[0] + t8[2] + t8[4] + t8[6]); out.n_tie_big = (int64_t)(t8[1] + t8[3] + t8[5] + t8[7]); }
        out.n_cand = cand_count;
        { static const int64_t zero_off[1] = {0}; out.off = zero_off; }
        if (want_entries && cand_count > 0) cand_bits_result(out);
        if (keep) {
            keep->cols = n_cols; keep->entries = n_entries; keep->cand = cand_count; keep->cand_entries = cand_entries; keep->ties = out.n_tie;
            if (want_entries) keep->cb_words = cand_bits_words();
            keep->valid = want_entries;
            keep->cand_per_contig = out.contig_n_cand;
        }
        kc.flush();
        if (int rc = e_k2.ms(&k_ms[0])) return rc;
        if (int rc = e_k3.ms(&k_ms[1])) return rc;
        return e_k3b.ms(&k_ms[2]);
    }

    // ---- K4 + the merge of the SNP lists + the SNP columns packed (they stay in d_pk for stage 4) ----
    DBuf d_keep;
    int64_t snp_count = 0, snp_entries = 0;       // what d_pk holds after finish_columns (HipSrOps::adopt_columns)
    // The entries of the SNP columns (.col's payload: 130 MB per C4 step) are read by nobody before the call's results are put together --
    // stage 4 takes the columns over on the device --, so with defer_entries they leave on a stream of their own once the block is
    // packed and are waited for in late_entries(), after stage 4 of the group has been queued and run
    bool defer_entries = false, entries_pending = false;
    int late_entries(hs::CvSnpSet& out) override {
        if (!entries_pending) return HS_OK;
        entries_pending = false;
        if (int rc = stream_wait(keep->side)) return rc;
        const char* hb = (const char*)h_pk.p;
        out.idx = (const int32_t*)(hb + pk_layout.idx); out.code = (const uint8_t*)(hb + pk_layout.code);
        return HS_OK;
    }
    int finish_columns(const hs::CvPartitionTest& t, bool want_entries, hs::CvSnpSet& out, float* k_ms) override {
        const int C = range_c1 - range_c0;
        const bool late = want_entries && defer_entries && keep != nullptr;
        entries_pending = false;
        out = hs::CvSnpSet();
        out.contig_n_snp.assign((size_t)C, 0);
        if (k_ms) *k_ms = 0;
        if ((int)t.contig_n_reads.size() != C) { set_error("finish_columns: partitions of another contig range"); return HS_EINVAL; }
        if (stream_late) stream = stream_late;      // (the host has waited for the column pass: nothing of it is in flight on the other stream)
        snp_count = 0; snp_entries = 0;
        static const int64_t zero_off[1] = {0};
        if (n_cols == 0 || C == 0) {
            pk_layout = pack_layout(0, 0);
            if (int rc = grow(d_pk, pk_layout.total)) return rc;
            hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, reinterpret_cast<uint4*>((char*)d_pk.p + pk_layout.off), 1ll, 0u);
            out.off = zero_off;
            return stream_wait(stream);
        }
        const int n = (int)n_cols;
        DBuf d_po, d_pso, d_ps;
        DBuf d_tab, d_pres, d_tab_off, d_ctg_nr, d_list;
        UploadPack pk_tab;      // one upload: the partitions and the table offsets (partition_test_launch adds its arrays and commits)
        pk_tab.add(t.part_off, d_po);
        pk_tab.add(t.part_state_off, d_pso);
        pk_tab.add(t.part_state, d_ps);
        if (int rc = grow(d_keep, (size_t)n)) return rc;
        EventPair e; if (int rc = e.init()) return rc;
        HS_HIP(ev_rec(e.a, stream));
        if (int rc = partition_test_launch(d_co.as<int64_t>(), d_ci.as<int32_t>(), d_cc.as<uint8_t>(), d_col_ctg.as<int32_t>(), d_k0.as<uint8_t>(),
                                           d_k1.as<uint8_t>(), d_c1.as<int32_t>(), d_cand.as<uint8_t>(), n, d_po, d_pso,
                                           d_ps, t.part_off.data(), t.contig_n_reads.data(), C, d_keep.as<uint8_t>(),
                                           stream, d_tab, d_pres, d_tab_off, d_ctg_nr, d_list, pk_tab, &kc, gathered_entries, (int64_t)t.part_state.size())) return rc;
        HS_HIP(ev_rec(e.b, stream));
        if (int rc = kc.begin(HS_K_SNP_SELECT, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_snp_bounds, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, stream, d_col_rec.as<hsdev::hs_colrec_dev>(), d_col_ctg.as<int32_t>(),
                           d_keep.as<uint8_t>(), n_cols, C, dev_snp_bounds());
        hipLaunchKernelGGL(hsdev::k_snp_flags, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, stream, d_col_rec.as<hsdev::hs_colrec_dev>(), d_col_ctg.as<int32_t>(),
                           d_keep.as<uint8_t>(), n_cols, C, dev_snp_bounds(), dev_ctg_snp());
        HS_HIP(hipGetLastError());
        if (int rc = kc.end(33 * n_cols, stream)) return rc;      // records in (twice) and out, the verdicts in
        if (int rc = flag_sums_launch(HS_COL_SNP, n_cols)) return rc;
        bool hinted = keep && keep->valid && keep->snp > 0 && hints_on();
        for (;;) {
            int64_t cap_snp, cap_snp_entries;
            if (!hinted) {
                if (int rc = fetch_info()) return rc;      // (the partition tables, uploads and lists of this scope are done with: it waits)
                cap_snp = host_header().n_flagged; cap_snp_entries = host_header().n_flagged_entries;
            } else { cap_snp = with_margin(keep->snp); cap_snp_entries = with_margin(keep->snp_entries); }
            if (int rc = pack_launch(HS_COL_SNP, n_cols, cap_snp, cap_snp_entries)) return rc;
            // the SNPs' records and offsets (and, for a caller that writes the .col file, their entries) into pinned memory, with the info block
            const PackLayout& L = pk_layout;
            if (int rc = grow(h_pk, std::max<size_t>(want_entries ? L.total : L.head, 256))) return rc;
            if (int rc = grow(h_info, info_bytes(C))) return rc;
            const long long* n_flagged = reinterpret_cast<const long long*>((const char*)d_info.p + offsetof(hsdev::ColumnsHeader, n_flagged));
            const long long* n_flagged_e = reinterpret_cast<const long long*>((const char*)d_info.p + offsetof(hsdev::ColumnsHeader, n_flagged_entries));
            Shipment sh;
            const char* base = (const char*)d_pk.p;
            sh.add_counted((char*)h_pk.p + L.rec, base + L.rec, n_flagged, 16, cap_snp);
            sh.add_counted((char*)h_pk.p + L.off, base + L.off, n_flagged, 8, cap_snp, 8);
            if (want_entries && !late) {
                sh.add_counted((char*)h_pk.p + L.idx, base + L.idx, n_flagged_e, 4, cap_snp_entries);
                sh.add_counted((char*)h_pk.p + L.code, base + L.code, n_flagged_e, 1, cap_snp_entries);
            }
            sh.add(h_info.p, d_info.p, info_bytes(C));
            if (int rc = kc.begin(HS_K_SHIP, stream)) return rc;
            if (int rc = sh.launch(stream)) return rc;
            if (int rc = kc.end(0, stream)) return rc;
            if (int rc = stream_wait(stream)) return rc;
            if (host_header().n_flagged <= cap_snp && host_header().n_flagged_entries <= cap_snp_entries) break;
            if (!hinted) { set_error("finish_columns: the packed SNP block does not hold the SNPs"); return HS_EINVAL; }
            hinted = false;      // (more SNPs than last time: once more with the counts known)
        }
        const int64_t n_snp = host_header().n_flagged, e_snp = host_header().n_flagged_entries;
        if (late && e_snp > 0) {      // the entries: queued on the side stream behind the packed block (which this stream has finished: the wait above)
            if (!keep->side) HS_HIP(hipStreamCreateWithFlags(&keep->side, hipStreamNonBlocking));
            const PackLayout& L = pk_layout;
            const char* base = (const char*)d_pk.p;
            // The copy engines take this one (130 MB per C4 step beside everything stage 4 ships: as a shipment kernel it held a thousand
            // wavefront slots while the link was busy; measured 15.1-15.6 ms per step with the payload against 16.0-16.2).
            // HS_LATE_ENTRIES=<n>: a shipment kernel with n workgroups instead
            static const char* mode = std::getenv("HS_LATE_ENTRIES");
            if (!(mode && std::atoi(mode) > 0)) {
                HS_HIP(hipMemcpyAsync((char*)h_pk.p + L.idx, base + L.idx, (size_t)e_snp * 4, hipMemcpyDeviceToHost, keep->side));
                HS_HIP(hipMemcpyAsync((char*)h_pk.p + L.code, base + L.code, (size_t)e_snp, hipMemcpyDeviceToHost, keep->side));
            } else {
                Shipment sh2;
                sh2.add((char*)h_pk.p + L.idx, base + L.idx, (size_t)e_snp * 4);
                sh2.add((char*)h_pk.p + L.code, base + L.code, (size_t)e_snp);
                if (int rc = sh2.launch(keep->side, std::atoi(mode))) return rc;
            }
            entries_pending = true;
        }
        std::memcpy(out.contig_n_snp.data(), host_ctg_snp(), (size_t)C * 4);
        out.n_snp = n_snp; out.n_entries = e_snp;
        snp_count = n_snp; snp_entries = e_snp;
        if (keep) { keep->snp = n_snp; keep->snp_entries = e_snp; }
        if (n_snp > 0) {
            const char* hb = (const char*)h_pk.p;
            out.rec = (const hs_colrec*)(hb + pk_layout.rec); out.off = (const int64_t*)(hb + pk_layout.off);
            if (want_entries && !late) { out.idx = (const int32_t*)(hb + pk_layout.idx); out.code = (const uint8_t*)(hb + pk_layout.code); }
        } else out.off = zero_off;
        kc.flush();
        return k_ms ? e.ms(k_ms) : HS_OK;
    }
    // ---- loop A on the device (hs_kernels_loopa.hip) on the candidates of the last extract_candidates() ----
    bool has_partition_pairs() const override { return true; }
    int partition_pairs(const std::vector<int8_t>& state, const std::vector<int32_t>& more, const std::vector<int32_t>& less, const std::vector<int64_t>& part_off,
                        const std::vector<int32_t>& part_n, const std::vector<int32_t>& pair_a, const std::vector<int32_t>& pair_b, const std::vector<float>& sigma3,
                        std::vector<int32_t>& out) override {
        const int n_pairs = (int)pair_a.size();
        out.assign((size_t)n_pairs * 8, 0);
        if (n_pairs == 0) return HS_OK;
        DBuf d_st, d_mo, d_le, d_po, d_pn, d_pa, d_pb, d_sg, d_out;
        UploadPack pk;
        pk.add(state, d_st); pk.add(more, d_mo); pk.add(less, d_le); pk.add(part_off, d_po); pk.add(part_n, d_pn); pk.add(pair_a, d_pa); pk.add(pair_b, d_pb); pk.add(sigma3, d_sg);
        if (int rc = pk.commit(stream)) return rc;
        if (int rc = d_out.alloc((size_t)n_pairs * 32)) return rc;
        if (int rc = hs_partition_pair_distance(d_st.as<int8_t>(), d_mo.as<int32_t>(), d_le.as<int32_t>(), d_po.as<int64_t>(), d_pn.as<int32_t>(), d_pa.as<int32_t>(),
                                                d_pb.as<int32_t>(), n_pairs, 2, d_sg.as<float>(), d_out.as<int32_t>(), stream)) return rc;
        return d2h_pinned(out.data(), d_out.p, (size_t)n_pairs * 32, stream);
    }
    // ---- loop A on the device (hs_kernels_loopa.hip) for the contigs of the range its tables hold; the others' candidates go to the host as bit sets ----
    // Opt-in, by measurement (round 6, profiles/r06_loop_a_split.txt): k_loop_a walks a candidate in 2.8 us (a lone wavefront issues one
    // instruction every four cycles, a candidate takes ~1 500 of them), a host core in 0.15 us; a launch lasts as long as its longest
    // contig, and every split of the C4 job between device and host -- by candidate count, by contig group -- made the step longer
    // (15.0 ms with everything on the host; 17.2 with the contigs of up to 300 candidates on the device, 18.0 with the first group's,
    // 28-30 with all contigs of up to 1 500), although the process's CPU time went down (183 -> 140 ms).
    // HS_LOOP_A_ON_DEVICE=1 (or "all"): every contig the kernel's tables hold; HS_LOOP_A_DEVICE_MAX=<n>: the contigs with at most n candidates
    // (HS_LOOP_A_DEVICE_MAX may be a list: one bound per contig group of a pipeline, the last one for the groups behind it -- the chain of a
    // group that the step does not wait for may be long)
    int loop_a_device_max() const {
        static const std::vector<int> v = []() {
            std::vector<int> r;
            const char* e = std::getenv("HS_LOOP_A_ON_DEVICE");
            if (e && e[0] == '0') { r.push_back(0); return r; }
            if (e && (e[0] == '1' || e[0] == 'a')) { r.push_back(0x7fffffff); return r; }
            const char* m = std::getenv("HS_LOOP_A_DEVICE_MAX");
            if (m) { for (const char* p = m; *p;) { r.push_back(std::atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; } }
            if (r.empty()) r.push_back(0);
            return r;
        }();
        const size_t g = order_ticket < 0 ? 0 : (size_t)order_ticket;
        return v[g < v.size() ? g : v.size() - 1];
    }
    hipEvent_t ev_cand = nullptr;
    int loop_a_plan(const int32_t* counts, int C) {
        static const int pool_div = []() { const char* e = std::getenv("HS_LOOP_A_POOL_DIV"); return e && std::atoi(e) > 0 ? std::atoi(e) : 6; }();
        std::vector<int32_t> n_reads((size_t)C);
        for (int c = 0; c < C; ++c) n_reads[(size_t)c] = b->contig_rec_off[(size_t)(range_c0 + c) + 1] - b->contig_rec_off[(size_t)(range_c0 + c)];
        const bool forced = keep && (int)keep->la_force_host.size() == C;
        return la_make_plan(counts, n_reads.data(), C, loop_a_device_max(), pool_div, forced ? keep->la_force_host.data() : nullptr, stream);
    }
    int loop_a_launch(int64_t cap_cand) {
        const char* cb = (const char*)d_cand_pk.p;
        LoopAIn in;
        in.rec = (const hsdev::hs_colrec_dev*)(cb + cand_layout.rec); in.off = (const int64_t*)(cb + cand_layout.off);
        in.idx = cand_layout.light ? d_ci.as<int32_t>() : (const int32_t*)(cb + cand_layout.idx);
        in.code = cand_layout.light ? d_cc.as<uint8_t>() : (const uint8_t*)(cb + cand_layout.code);
        in.len = cand_layout.light ? (const int32_t*)(cb + cand_layout.len) : nullptr;
        in.header = dev_header(); in.ctg_n = dev_ctg_n(); in.contig_rec_off = b->d_contig_rec_off.as<int32_t>(); in.rank_end = b->d_rank_end.as<int2>();
        in.orig_of = b->d_orig_of.as<int32_t>(); in.c0 = range_c0;
        return la_queue(in, range_c1 - range_c0, cap_cand, with_margin(keep ? keep->la_span : 0), keep && keep->cand > 0 ? keep->cand : cap_cand, kc, stream);
    }
    // the partitions loop A left on the device (after extract_candidates has returned and the host has walked its own contigs)
    int collect_partitions(hs::CvLoopAResult& out) override {
        if (!la_launched) { out = hs::CvLoopAResult(); return HS_OK; }
        const int C = range_c1 - range_c0;
        int64_t span = 0;
        if (int rc = la_collect(C, out, kc, stream, &span)) return rc;
        if (keep) {
            keep->la_span = span;
            for (int c = 0; c < C; ++c) if (out.failed[(size_t)c]) { if ((int)keep->la_force_host.size() != C) keep->la_force_host.assign((size_t)C, 0); keep->la_force_host[(size_t)c] = 1; }
        }
#ifdef HS_LA_DIAG
        {
            unsigned long long dg[10];
            if (int rc = d2h_pinned(dg, d_la_diag.p, sizeof dg, stream)) return rc;
            std::fprintf(stderr, "[hs la] cycles: head %llu, compare %llu, emulator %llu, verdict+evict %llu, augment %llu, create %llu, end %llu; candidates %llu, emulator lanes %llu\n",
                         dg[0], dg[1], dg[2], dg[3], dg[4], dg[5], dg[7], dg[8], dg[9]);
        }
#endif
        kc.flush();
        return HS_OK;
    }
    ~HipCvOps() {
        // (an error between finish_columns and late_entries: the entries' copy on the side stream still writes the group's pinned block)
        if (entries_pending && keep && keep->side) (void)stream_wait(keep->side);
        if (ev_cand) EventPair::cache().push_back(ev_cand);
    }
};

