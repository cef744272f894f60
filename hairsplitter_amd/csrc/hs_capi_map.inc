// hs_capi_map.inc -- part of hs_capi.hip: the read mapper (include/hairsplitter_hip.h: hs_map_index_create, hs_map_reads, hs_map_to_batch). Kernels
// in hs_kernels_map.hip, the rule and the host half in hs_map_host.h / hs_map_host.cpp. An index call waits twice (the number of minimizers, which
// sizes the entries; the end), a map call three times (the minimizers, then the hits -- each total sizes what follows --, then the records: one
// block, one shipment). A split call (hs_map_reads_split) waits three times as well: its segments are compacted on the device and leave in the same
// shipment, their number read there; so does an anchored call (hs_map_reads_anchored), whose anchors leave the same way. Sequences go up by the
// runtime's upload_pageable. Launches are accounted under HS_K_OTHER. A map call is a MapCall: one method per stage, each entry the stages it uses.
// The three *_to_batch entries share ToBatch: one argument check, one route through the realign job (hs_capi_realign.inc), one hand-over.
struct hs_map_index {
    hs_map_params params{};
    int32_t n_contigs = 0, bucket_bits = 0;
    int64_t n_entries = 0;
    std::vector<int64_t> contig_off;
    DBuf d_contig_off, d_bucket_off, d_e_h, d_e_c, d_e_ts;
};

namespace {

// zero bytes behind every array a call uploads: a load a little past an end finds zeros, not a neighbour's block
static const size_t MAP_SLACK = 16;

// offsets of a job's sequences: ascending from 0, every sequence below 2^31 bases, the whole below 2^38
static int map_check_offsets(const int64_t* off, int32_t n, const char* what) {
    bool ok = off[0] == 0;
    for (int32_t i = 0; ok && i < n; ++i) ok = off[i + 1] >= off[i] && off[i + 1] - off[i] <= 0x7fffffff;
    if (!ok || off[n] > ((int64_t)1 << 38)) { set_error(std::string(what) + ": offsets must ascend from 0, a sequence holds at most 2^31 - 1 bases and a call 2^38"); return HS_EINVAL; }
    return HS_OK;
}

// the minimizers of resident sequences, (sequence, position) ascending: count, scan, (one wait: the total), write
struct MapMinimizersDev {
    DBuf h, ps, seq, blk_cnt, blk_off, scan;
    int64_t n = 0;
    int run(const uint8_t* d_seq, const int64_t* d_off, int32_t n_seqs, int64_t total, const hs_map_params& p, hipStream_t st) {
        n = 0;
        const int64_t n_blk = (total + 255) / 256;
        if (n_blk > 0) {
            if (int rc = blk_cnt.alloc((size_t)n_blk * 4)) return rc;
            if (int rc = blk_off.alloc(((size_t)n_blk + 1) * 8)) return rc;
            hipLaunchKernelGGL(hsdev::k_map_minimizers<false>, dim3((unsigned)n_blk), dim3(256), 0, st, d_seq, d_off, n_seqs, (long long)total, p.k, p.w, blk_cnt.as<int32_t>(),
                               (const int64_t*)nullptr, 0ll, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr);
            HS_HIP(hipGetLastError());
            if (int rc = exclusive_scan_launch(blk_cnt.as<int32_t>(), (int)n_blk, blk_off.as<int64_t>(), scan, st)) return rc;
            if (int rc = copy_d2h(&n, blk_off.as<int64_t>() + n_blk, 8, st)) return rc;
            if (n < 0 || n > total) { set_error("map: the device's minimizer count does not fit the sequences"); return HS_EHIP; }
        }
        for (DBuf* b : {&h, &ps, &seq}) if (int rc = b->alloc((size_t)std::max<int64_t>(n, 1) * 4)) return rc;
        if (n > 0) {
            hipLaunchKernelGGL(hsdev::k_map_minimizers<true>, dim3((unsigned)n_blk), dim3(256), 0, st, d_seq, d_off, n_seqs, (long long)total, p.k, p.w, (int32_t*)nullptr,
                               blk_off.as<int64_t>(), (long long)n, h.as<uint32_t>(), ps.as<uint32_t>(), seq.as<int32_t>());
            HS_HIP(hipGetLastError());
        }
        return HS_OK;
    }
};

// The parts of a map call's output block: the per-read records under the names hs_map_result gives them, then what a call clears -- n_skipped,
// the wide route's counter, the word of the largest read -- side by side (one clearing). Up to `shipped` the block goes to the host in one
// shipment and lands there at the same offsets; behind it lies the wide route's list [R].
// An anchored call (hs_map_reads_anchored) adds n_best, n_chain and n_supported per read at the end of the shipped part and, behind the list, the
// anchor count of every read and the best key the vote leaves for k_map_anchors (8 bytes per read); its anchors lie in blocks of their own.
// A split call (hs_map_reads_split) has no per-read records: in their place round 0's vote per read (votes, second -- cleared with the rest, a read
// without a hit keeps the zeros) and, behind the shipped part, the segment count of every read (cleared too). Its segments lie in blocks of their own.
struct MapWork {
    int64_t contig, strand, qstart, qend, tstart, tend, votes, second, n_minimizers, n_hits, n_skipped, wide_count, max_hits, shipped, wide_list, total_bytes;
    int64_t clear_from, clear_to, seg_count;
    int64_t n_best, n_chain, n_supported, anc_count, best_key;      // an anchored call (hs_map_reads_anchored) only
};
static MapWork map_work(int32_t n_reads, bool split = false, bool anchored = false) {
    const int64_t R = n_reads;
    MapWork m{};
    WorkParts p;
    if (!split) {
        m.contig = p.take(R * 4); m.strand = p.take(R); m.qstart = p.take(R * 4); m.qend = p.take(R * 4); m.tstart = p.take(R * 4); m.tend = p.take(R * 4);
        m.votes = p.take(R * 4); m.second = p.take(R * 4);
    }
    m.n_minimizers = p.take(R * 4); m.n_hits = p.take(R * 8);
    m.clear_from = p.o;
    if (split) { m.votes = p.take(R * 4); m.second = p.take(R * 4); }
    m.n_skipped = p.take(R * 4); m.wide_count = p.take(4); m.max_hits = p.take(16);
    if (anchored) { m.n_best = p.take(R * 4); m.n_chain = p.take(R * 4); m.n_supported = p.take(R * 4); }      // (k_map_anchors writes every read's: nothing to clear)
    m.shipped = p.o;
    if (split) m.seg_count = p.take(R * 4);
    m.clear_to = p.o;
    m.wide_list = p.take(R * 4);
    if (anchored) { m.anc_count = p.take(R * 4); m.best_key = p.take(R * 8); }
    m.total_bytes = p.o;
    return m;
}

// an array of a result struct: one element of room at least (as the destroy functions and the callers expect), zeroed, then n elements of src where given
template <class T> static bool map_room(T*& dst, size_t n, const void* src = nullptr) {
    dst = (T*)std::calloc(std::max<size_t>(1, n), sizeof(T));
    if (dst && n && src) std::memcpy(dst, src, n * sizeof(T));
    return dst != nullptr;
}

// One map call (hs_map_reads, hs_map_reads_split, hs_map_reads_anchored): its buffers, the output block, the kernel clock and the events, a method per
// stage in the order the entries run them -- begin (upload, minimizers; one wait), hits (one wait), vote or vote_split, anchors, ship (one wait) --
// and the builders that turn the shipped block into the result structs.
struct MapCall {
    const std::string who;
    const hs_map_index* const index;
    const uint8_t* const h_read_seq;
    const int64_t* const h_read_off;
    const int32_t n_reads;
    const hs_map_split_params* split = nullptr;        // set by the entry before begin(): they decide the block's layout
    const hs_map_anchor_params* anchor = nullptr;
    const hipStream_t st = nullptr;
    const size_t seg_bytes = (size_t)HS_MAP_SEG_WORDS * 4;
    size_t R = 0;
    int64_t total = 0, M = 0, H = 0, max_hits = 0, slab_keys = 0, seg_cap = 0, anc_cap = 0;
    int wide_blocks = 0;
    KernelClock kc;
    EventPair ev_mz, ev_hits, ev_vote, ev_anc;
    DBuf d_seq, d_off, d_mz_off, d_cnt, d_hit_off, d_scan, d_key, d_qa, d_t, d_slabs, d_out, d_seg_off, d_staged, d_segs, d_stage_q, d_stage_t, d_anc_off, d_anc_q, d_anc_t;
    HBuf h_out, h_seg_off, h_segs, h_anc_off, h_anc_q, h_anc_t;
    MapMinimizersDev mz;
    MapWork w{};
    char* out = nullptr;
    hsdev::MapVoteArgs A{};

    MapCall(const char* who_, const hs_map_index* index_, const uint8_t* seq, const int64_t* off, int32_t n) : who(who_), index(index_), h_read_seq(seq), h_read_off(off), n_reads(n) {}
    int bad_arguments() const { set_error(who + ": bad arguments"); return HS_EINVAL; }
    // the device and the arguments every entry shares (outs_ok: the entry's own out-pointers, which it nulls next)
    int check(bool outs_ok) const {
        if (int rc = require_device()) return rc;
        if (!index || !outs_ok || !h_read_off || n_reads < 0) return bad_arguments();
        return HS_OK;
    }
    // the parameters of a split or anchored call, the reads' offsets
    int check_job() const {
        if (anchor && !hs::map_anchor_params_valid(*anchor)) { set_error(who + ": anchor parameters out of range (spacing >= 1)"); return HS_EINVAL; }
        if (split && !hs::map_split_params_valid(*split)) { set_error(who + ": split parameters out of range (max_segments 1..8, min_votes >= 1, min_span >= 0, max_gap >= 0)"); return HS_EINVAL; }
        if (int rc = map_check_offsets(h_read_off, n_reads, who.c_str())) return rc;
        if (h_read_off[n_reads] > 0 && !h_read_seq) return bad_arguments();
        return HS_OK;
    }
    // the stages of an entry, with the exceptions of the host's containers turned into its error
    template <class Stages> int run(Stages stages) {
        try { return stages(); } catch (const std::exception& e) { set_error(who + ": " + e.what()); return HS_EINVAL; }
    }

    // ---- the reads up, their minimizers and every read's range of them (one wait: their total) ----
    int begin() {
        if (int rc = check_job()) return rc;
        R = (size_t)n_reads; total = h_read_off[n_reads];
        for (EventPair* e : {&ev_mz, &ev_hits, &ev_vote, &ev_anc}) if (int rc = e->init()) return rc;
        if (int rc = upload_pageable(d_seq, h_read_seq, (size_t)total, 0, MAP_SLACK)) return rc;
        if (int rc = upload_pageable(d_off, h_read_off, (R + 1) * 8, 0, MAP_SLACK)) return rc;
        int64_t mz_bytes = total;
        if (int rc = timed_launch(kc, ev_mz, st, mz_bytes, [&]() -> int {
                if (int rc = mz.run(d_seq.as<uint8_t>(), d_off.as<int64_t>(), n_reads, total, index->params, st)) return rc;
                mz_bytes += 12 * mz.n;
                if (mz.n > 0x7fffffff - HS_SCAN_TILE) { set_error(who + ": more than 2^31 read minimizers in one call: map the reads in several calls"); return HS_EINVAL; }
                if (int rc = d_mz_off.alloc((R + 1) * 8)) return rc;
                hipLaunchKernelGGL(hsdev::k_map_seq_ranges, dim3((unsigned)(R / 256 + 1)), dim3(256), 0, st, mz.seq.as<int32_t>(), (long long)mz.n, n_reads, d_mz_off.as<int64_t>());
                HS_HIP(hipGetLastError());
                return HS_OK; })) return rc;
        M = mz.n;
        return HS_OK;
    }

    // ---- the output block; occ of every minimizer, the hits' offsets, (one wait: their total and the most a read has), the hits ----
    int hits() {
        const hs_map_params& prm = index->params;
        w = map_work(n_reads, split != nullptr, anchor != nullptr);
        if (int rc = d_out.alloc((size_t)w.total_bytes)) return rc;
        out = (char*)d_out.p;
        if (int rc = d_cnt.alloc((size_t)std::max<int64_t>(M, 1) * 4)) return rc;
        if (int rc = d_hit_off.alloc(((size_t)M + 1) * 8)) return rc;
        hsdev::MapIndexDev X{index->d_bucket_off.as<int64_t>(), index->d_e_h.as<uint32_t>(), index->d_e_c.as<int32_t>(), index->d_e_ts.as<uint32_t>(),
                             (uint32_t)(((int64_t)1 << index->bucket_bits) - 1), (long long)index->n_entries, index->d_contig_off.as<int64_t>(), index->n_contigs};
        int64_t hit_bytes = 8 * M;
        return timed_launch(kc, ev_hits, st, hit_bytes, [&]() -> int {
                HS_HIP(hipMemsetAsync(out + w.clear_from, 0, (size_t)(w.clear_to - w.clear_from), st));      // (n_skipped, the wide counter, the largest read; a split call's vote and counts)
                const unsigned grid_m = (unsigned)((M + 255) / 256);
                if (M > 0) hipLaunchKernelGGL(hsdev::k_map_hits_count, dim3(grid_m), dim3(256), 0, st, X, mz.h.as<uint32_t>(), mz.seq.as<int32_t>(), (long long)M, n_reads, prm.max_occ,
                                              d_cnt.as<int32_t>(), (int32_t*)(out + w.n_skipped));
                if (int rc = exclusive_scan_launch(d_cnt.as<int32_t>(), (int)M, d_hit_off.as<int64_t>(), d_scan, st)) return rc;
                if (R) hipLaunchKernelGGL(hsdev::k_map_read_hits, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, d_mz_off.as<int64_t>(), d_hit_off.as<int64_t>(), n_reads,
                                          (int64_t*)(out + w.n_hits), (int32_t*)(out + w.n_minimizers), (unsigned long long*)(out + w.max_hits));
                HS_HIP(hipGetLastError());
                HS_HIP(HS_COPY_ASYNC(&max_hits, out + w.max_hits, 8, hipMemcpyDeviceToHost, st));
                if (int rc = copy_d2h(&H, d_hit_off.as<int64_t>() + M, 8, st)) return rc;
                if (H < 0 || max_hits < 0 || max_hits > H) { set_error(who + ": the device's hit counts do not fit the minimizers"); return HS_EHIP; }
                if (max_hits > ((int64_t)1 << 28)) { set_error(who + ": a read with more than 2^28 hits: lower max_occ"); return HS_EINVAL; }
                hit_bytes += 2 * 16 * H;
                if (int rc = d_key.alloc((size_t)std::max<int64_t>(H, 1) * 8)) return rc;
                if (int rc = d_qa.alloc((size_t)std::max<int64_t>(H, 1) * 4)) return rc;
                if (int rc = d_t.alloc((size_t)std::max<int64_t>(H, 1) * 4)) return rc;
                if (M > 0 && H > 0) hipLaunchKernelGGL(hsdev::k_map_hits_fill, dim3(grid_m), dim3(256), 0, st, X, mz.h.as<uint32_t>(), mz.ps.as<uint32_t>(), mz.seq.as<int32_t>(), (long long)M,
                                                       d_off.as<int64_t>(), n_reads, prm, d_cnt.as<int32_t>(), d_hit_off.as<int64_t>(), (long long)H, d_key.as<uint64_t>(), d_qa.as<int32_t>(),
                                                       d_t.as<int32_t>());
                HS_HIP(hipGetLastError());
                return HS_OK; });
    }

    // what both votes take: the wide route's slabs and the arguments (a split call's block has no per-read records: the six stay null)
    int vote_args() {
        slab_keys = max_hits <= HS_MAP_LDS_KEYS ? 2 : hsdev::pow2_at_least((int)max_hits);      // (2: the list stays empty)
        wide_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(HS_MAP_WIDE_BLOCKS, ((int64_t)1 << 28) / slab_keys));
        if (int rc = d_slabs.alloc((size_t)slab_keys * 8 * (size_t)wide_blocks)) return rc;
        A.mz_off = d_mz_off.as<int64_t>(); A.hit_off = d_hit_off.as<int64_t>(); A.hit_key = d_key.as<uint64_t>(); A.hit_qa = d_qa.as<int32_t>(); A.hit_t = d_t.as<int32_t>(); A.n_hits = H;
        A.read_off = d_off.as<int64_t>(); A.contig_off = index->d_contig_off.as<int64_t>(); A.n_contigs = index->n_contigs; A.n_reads = n_reads; A.P = index->params;
        if (!split) {
            A.contig = (int32_t*)(out + w.contig); A.strand = (uint8_t*)(out + w.strand); A.qstart = (int32_t*)(out + w.qstart); A.qend = (int32_t*)(out + w.qend);
            A.tstart = (int32_t*)(out + w.tstart); A.tend = (int32_t*)(out + w.tend);
        }
        A.votes = (int32_t*)(out + w.votes); A.second = (int32_t*)(out + w.second);
        A.wide_list = (int32_t*)(out + w.wide_list); A.wide_count = (int32_t*)(out + w.wide_count);
        if (anchor) A.best_key = (uint64_t*)(out + w.best_key);
        return HS_OK;
    }
    // ---- the vote: LDS route for every read, the scratch route for the list it leaves ----
    int vote() {
        if (int rc = vote_args()) return rc;
        return timed_launch(kc, ev_vote, st, 2 * 16 * H + 30 * (int64_t)R, [&]() -> int {
                if (R) hipLaunchKernelGGL(hsdev::k_map_vote, dim3((unsigned)R), dim3(256), 0, st, A);
                hipLaunchKernelGGL(hsdev::k_map_vote_wide, dim3((unsigned)wide_blocks), dim3(256), 0, st, A, d_slabs.as<uint64_t>(), (long long)slab_keys);
                HS_HIP(hipGetLastError());
                return HS_OK; });
    }
    // ---- a split call's vote: the rounds per read into a staging of max_segments per read, the counts' scan, the compaction ----
    int vote_split() {
        if (int rc = vote_args()) return rc;
        seg_cap = (int64_t)R * split->max_segments;
        if (int rc = d_seg_off.alloc((R + 1) * 8)) return rc;
        if (int rc = d_staged.alloc((size_t)std::max<int64_t>(seg_cap, 1) * seg_bytes)) return rc;
        if (int rc = d_segs.alloc((size_t)std::max<int64_t>(seg_cap, 1) * seg_bytes + MAP_SLACK)) return rc;
        hsdev::MapSplitArgs B{};
        B.S = *split; B.seg_count = (int32_t*)(out + w.seg_count); B.staged = d_staged.as<int32_t>(); B.read_votes = A.votes; B.read_second = A.second;
        return timed_launch(kc, ev_vote, st, 2 * 16 * H + 30 * (int64_t)R, [&]() -> int {
                if (R) hipLaunchKernelGGL(hsdev::k_map_vote_split, dim3((unsigned)R), dim3(256), 0, st, A, B);
                hipLaunchKernelGGL(hsdev::k_map_vote_split_wide, dim3((unsigned)wide_blocks), dim3(256), 0, st, A, B, d_slabs.as<uint64_t>(), (long long)slab_keys);
                HS_HIP(hipGetLastError());
                if (int rc = exclusive_scan_launch(B.seg_count, n_reads, d_seg_off.as<int64_t>(), d_scan, st)) return rc;
                if (seg_cap > 0) hipLaunchKernelGGL(hsdev::k_map_seg_compact, dim3((unsigned)((seg_cap + 255) / 256)), dim3(256), 0, st, B.seg_count, d_seg_off.as<int64_t>(),
                                                    d_staged.as<int32_t>(), n_reads, split->max_segments, (long long)seg_cap, d_segs.as<int32_t>());
                HS_HIP(hipGetLastError());
                return HS_OK; });
    }
    // ---- an anchored call: the cut points of every read staged at its upper bound, the counts' scan, the compaction ----
    int anchors() {
        anc_cap = hs::map_anchor_stage_at(total, (int64_t)R, anchor->spacing);
        if (anc_cap > 0x7fffffff) { set_error(who + ": room for more than 2^31 anchors in one call: map the reads in several calls"); return HS_EINVAL; }
        for (DBuf* b : {&d_stage_q, &d_stage_t, &d_anc_q, &d_anc_t}) if (int rc = b->alloc((size_t)std::max<int64_t>(anc_cap, 1) * 4 + MAP_SLACK)) return rc;
        if (int rc = d_anc_off.alloc((R + 1) * 8)) return rc;
        hsdev::MapAnchorArgs B2{};
        B2.P = *anchor; B2.stage_q = d_stage_q.as<int32_t>(); B2.stage_t = d_stage_t.as<int32_t>(); B2.stage_cap = (long long)anc_cap;
        B2.anc_count = (int32_t*)(out + w.anc_count); B2.n_best = (int32_t*)(out + w.n_best); B2.n_chain = (int32_t*)(out + w.n_chain); B2.n_supported = (int32_t*)(out + w.n_supported);
        return timed_launch(kc, ev_anc, st, 16 * H + 8 * anc_cap + 24 * (int64_t)R, [&]() -> int {
                if (R) hipLaunchKernelGGL(hsdev::k_map_anchors, dim3((unsigned)R), dim3(256), 0, st, A, B2);
                HS_HIP(hipGetLastError());
                if (int rc = exclusive_scan_launch(B2.anc_count, n_reads, d_anc_off.as<int64_t>(), d_scan, st)) return rc;
                if (R) hipLaunchKernelGGL(hsdev::k_map_anchor_compact, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, B2.anc_count, d_anc_off.as<int64_t>(), d_off.as<int64_t>(), n_reads,
                                          anchor->spacing, d_stage_q.as<int32_t>(), d_stage_t.as<int32_t>(), (long long)anc_cap, (long long)anc_cap, d_anc_q.as<int32_t>(), d_anc_t.as<int32_t>());
                HS_HIP(hipGetLastError());
                return HS_OK; });
    }
    // ---- the records: one shipment to pinned blocks (one wait). Segments and anchors leave in it too, their number read on the device when it runs
    // (the host blocks have room for the most there can be) ----
    int ship() {
        if (int rc = h_out.alloc((size_t)w.shipped)) return rc;
        Shipment sh;
        sh.add(h_out.p, out, (size_t)w.shipped);
        if (split) {
            if (int rc = h_seg_off.alloc((R + 1) * 8 + 16)) return rc;
            if (int rc = h_segs.alloc((size_t)std::max<int64_t>(seg_cap, 1) * seg_bytes + MAP_SLACK)) return rc;
            sh.add(h_seg_off.p, d_seg_off.p, (R + 1) * 8);
            if (seg_cap > 0) sh.add_counted(h_segs.p, d_segs.p, (const long long*)(d_seg_off.as<int64_t>() + R), seg_bytes, (long long)seg_cap);
        }
        if (anchor) {
            if (int rc = h_anc_off.alloc((R + 1) * 8 + 16)) return rc;
            for (HBuf* b : {&h_anc_q, &h_anc_t}) if (int rc = b->alloc((size_t)std::max<int64_t>(anc_cap, 1) * 4 + MAP_SLACK)) return rc;
            sh.add(h_anc_off.p, d_anc_off.p, (R + 1) * 8);
            if (anc_cap > 0) {
                sh.add_counted(h_anc_q.p, d_anc_q.p, (const long long*)(d_anc_off.as<int64_t>() + R), 4, (long long)anc_cap);
                sh.add_counted(h_anc_t.p, d_anc_t.p, (const long long*)(d_anc_off.as<int64_t>() + R), 4, (long long)anc_cap);
            }
        }
        if (int rc = sh.launch(st)) return rc;
        if (int rc = stream_wait(st)) return rc;
        kc.flush();
        return HS_OK;
    }

    // ---- the builders: the shipped block as the caller's structs ----
    const char* shipped(int64_t at) const { return (const char*)h_out.p + at; }
    int out_of_memory() const { set_error(who + ": out of memory"); return HS_EINVAL; }
    // the per-call statistics hs_map_result and hs_map_segments share
    template <class T> void statistics(T* r) {
        r->n_wide = *(const int32_t*)shipped(w.wide_count); r->total_minimizers = M; r->total_hits = H;
        float ms = 0;
        if (ev_mz.ms(&ms) == HS_OK) r->t_minimizers_ms = ms;
        if (ev_hits.ms(&ms) == HS_OK) r->t_hits_ms = ms;
        if (ev_vote.ms(&ms) == HS_OK) r->t_vote_ms = ms;
    }
    int make_result(hs_map_result** result) {
        hs_map_result* r = (hs_map_result*)std::calloc(1, sizeof(hs_map_result));
        if (!r) return out_of_memory();
        r->n_reads = n_reads;
        const bool ok = map_room(r->contig, R, shipped(w.contig)) && map_room(r->strand, R, shipped(w.strand)) && map_room(r->qstart, R, shipped(w.qstart))
                        && map_room(r->qend, R, shipped(w.qend)) && map_room(r->tstart, R, shipped(w.tstart)) && map_room(r->tend, R, shipped(w.tend))
                        && map_room(r->votes, R, shipped(w.votes)) && map_room(r->second, R, shipped(w.second)) && map_room(r->n_minimizers, R, shipped(w.n_minimizers))
                        && map_room(r->n_skipped, R, shipped(w.n_skipped)) && map_room(r->n_hits, R, shipped(w.n_hits));
        if (!ok) { hs_map_result_destroy(r); return out_of_memory(); }
        statistics(r);
        *result = r;
        return HS_OK;
    }
    int make_segments(hs_map_segments** segments) {
        const int64_t* so = (const int64_t*)h_seg_off.p;
        const int64_t S = so[R];
        bool ok = so[0] == 0 && S >= 0 && S <= seg_cap;
        for (size_t i = 0; ok && i < R; ++i) ok = so[i + 1] >= so[i] && so[i + 1] - so[i] <= split->max_segments;
        if (!ok) { set_error(who + ": the device's segment counts do not fit the reads"); return HS_EHIP; }
        hs_map_segments* g = (hs_map_segments*)std::calloc(1, sizeof(hs_map_segments));
        if (!g) return out_of_memory();
        g->n_reads = n_reads; g->n_segments = S;
        ok = map_room(g->seg_off, R + 1, so) && map_room(g->strand, (size_t)S);
        for (int32_t** a : {&g->read, &g->contig, &g->qstart, &g->qend, &g->tstart, &g->tend, &g->votes, &g->second, &g->round}) ok = ok && map_room(*a, (size_t)S);
        ok = ok && map_room(g->n_minimizers, R, shipped(w.n_minimizers)) && map_room(g->n_skipped, R, shipped(w.n_skipped)) && map_room(g->n_hits, R, shipped(w.n_hits))
             && map_room(g->read_votes, R, shipped(w.votes)) && map_room(g->read_second, R, shipped(w.second));
        if (!ok) { hs_map_segments_destroy(g); return out_of_memory(); }
        const int32_t* rec = (const int32_t*)h_segs.p;
        for (int64_t i = 0; i < S; ++i, rec += HS_MAP_SEG_WORDS) {
            g->read[i] = rec[0]; g->contig[i] = rec[1]; g->strand[i] = (uint8_t)rec[2]; g->qstart[i] = rec[3]; g->qend[i] = rec[4]; g->tstart[i] = rec[5]; g->tend[i] = rec[6];
            g->votes[i] = rec[7]; g->second[i] = rec[8]; g->round[i] = rec[9];
        }
        statistics(g);
        *segments = g;
        return HS_OK;
    }
    int make_anchors(hs_map_anchors** anchors) {
        const int64_t* ao = (const int64_t*)h_anc_off.p;
        const int64_t N = ao[R];
        bool ok = ao[0] == 0 && N >= 0 && N <= anc_cap;
        for (size_t i = 0; ok && i < R; ++i) ok = ao[i + 1] >= ao[i] && ao[i + 1] - ao[i] <= hs::map_anchor_bound(h_read_off[i + 1] - h_read_off[i], anchor->spacing);
        if (!ok) { set_error(who + ": the device's anchor counts do not fit the reads"); return HS_EHIP; }
        hs_map_anchors* a = (hs_map_anchors*)std::calloc(1, sizeof(hs_map_anchors));
        if (!a) return out_of_memory();
        a->n_reads = n_reads; a->n_anchors = N;
        ok = map_room(a->anc_off, R + 1, ao) && map_room(a->anc_q, (size_t)N, h_anc_q.p) && map_room(a->anc_t, (size_t)N, h_anc_t.p)
             && map_room(a->n_best, R, shipped(w.n_best)) && map_room(a->n_chain, R, shipped(w.n_chain)) && map_room(a->n_supported, R, shipped(w.n_supported));
        if (!ok) { hs_map_anchors_destroy(a); return out_of_memory(); }
        float ms = 0;
        if (ev_anc.ms(&ms) == HS_OK) a->t_anchors_ms = ms;
        *anchors = a;
        return HS_OK;
    }
};

// the mapped reads of a result as the intervals of the realign job; with `an`, every interval's anchors beside them
struct MappedIntervals {
    std::vector<int32_t> read, contig, qs, qe, ts, te, anc_q, anc_t;
    std::vector<uint8_t> strand;
    std::vector<int64_t> anc_off{0};
    MappedIntervals(const hs_map_result* mr, const hs_map_anchors* an) {
        for (int32_t i = 0; i < mr->n_reads; ++i) {
            if (mr->contig[i] < 0) continue;
            read.push_back(i); contig.push_back(mr->contig[i]); strand.push_back(mr->strand[i]);
            qs.push_back(mr->qstart[i]); qe.push_back(mr->qend[i]); ts.push_back(mr->tstart[i]); te.push_back(mr->tend[i]);
            if (!an) continue;
            anc_q.insert(anc_q.end(), an->anc_q + an->anc_off[i], an->anc_q + an->anc_off[i + 1]);
            anc_t.insert(anc_t.end(), an->anc_t + an->anc_off[i], an->anc_t + an->anc_off[i + 1]);
            anc_off.push_back((int64_t)anc_q.size());
        }
    }
};

// what a *_to_batch entry got from its map call: handed to the caller's pointers once the batch stands, destroyed on any other exit (and where the
// caller gave no pointer)
struct MapOwned {
    hs_map_result* result = nullptr; hs_map_segments* segments = nullptr; hs_map_anchors* anchors = nullptr;
    ~MapOwned() { hs_map_result_destroy(result); hs_map_segments_destroy(segments); hs_map_anchors_destroy(anchors); }
    template <class T> static void hand(T*& mine, T** theirs) { if (theirs) { *theirs = mine; mine = nullptr; } }
};

// the sequences of a *_to_batch call and where its outputs go (any of the last four may be NULL)
struct ToBatch {
    const uint8_t* h_contig_seq; const int64_t* h_contig_off; int32_t n_contigs; const uint8_t* h_read_seq; const int64_t* h_read_off; int32_t n_reads, pad;
    hs_cv_batch** batch; hs_realign_records** records; hs_map_result** result; hs_map_segments** segments; hs_map_anchors** anchors;
    // the arguments the three entries check alike; the out-pointers null until the batch stands
    int check(const char* who, const hs_map_index* index) const {
        if (int rc = require_device()) return rc;
        if (!index || !batch || !h_contig_off || n_contigs != index->n_contigs) { set_error(std::string(who) + ": bad arguments (the contigs are the index's)"); return HS_EINVAL; }
        *batch = nullptr;
        if (records) *records = nullptr;
        if (result) *result = nullptr;
        if (segments) *segments = nullptr;
        if (anchors) *anchors = nullptr;
        return HS_OK;
    }
    // the one route from intervals (anc_off NULL: without anchors) through the realign job to the batch; then `got` changes hands
    int realign(const int32_t* iv_read, const int32_t* iv_contig, const uint8_t* iv_strand, const int32_t* qs, const int32_t* qe, const int32_t* ts, const int32_t* te, int64_t n_intervals,
                const int64_t* anc_off, const int32_t* anc_q, const int32_t* anc_t, MapOwned& got) const {
        hs_realign_records* rec = nullptr;
        if (int rc = realign_job(anc_off ? "hs_realign_intervals_anchored" : "hs_realign_intervals", h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, iv_read, iv_contig,
                                 iv_strand, qs, qe, ts, te, (int32_t)n_intervals, pad, anc_off, anc_q, anc_t, &rec, batch)) return rc;
        if (records) *records = rec; else hs_realign_records_destroy(rec);
        MapOwned::hand(got.result, result); MapOwned::hand(got.segments, segments); MapOwned::hand(got.anchors, anchors);
        return HS_OK;
    }
    int realign(const MappedIntervals& iv, bool anchored, MapOwned& got) const {
        return realign(iv.read.data(), iv.contig.data(), iv.strand.data(), iv.qs.data(), iv.qe.data(), iv.ts.data(), iv.te.data(), (int64_t)iv.read.size(),
                       anchored ? iv.anc_off.data() : nullptr, iv.anc_q.data(), iv.anc_t.data(), got);
    }
};

}  // namespace

extern "C" {

int32_t hs_map_lds_capacity(void) { return HS_MAP_LDS_KEYS; }

void hs_map_index_destroy(hs_map_index* index) { delete index; }

int hs_map_index_create(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const hs_map_params* params, hs_map_index** index) {
    if (int rc = require_device()) return rc;
    if (!index || !h_contig_off || n_contigs < 0) { set_error("hs_map_index_create: bad arguments"); return HS_EINVAL; }
    *index = nullptr;
    const hs_map_params prm = params ? *params : hs_map_params_default();
    if (!hs::map_params_valid(prm)) { set_error("hs_map_index_create: parameters out of range (k 5..16, w 1..32, max_occ >= 1, band_log2 0..30, min_votes >= 1, extend 0|1, bucket_bits -1..26)"); return HS_EINVAL; }
    if (int rc = map_check_offsets(h_contig_off, n_contigs, "hs_map_index_create")) return rc;
    const int64_t total = h_contig_off[n_contigs];
    if (total > 0 && !h_contig_seq) { set_error("hs_map_index_create: bad arguments"); return HS_EINVAL; }
    try {
        std::unique_ptr<hs_map_index> ix(new hs_map_index());
        ix->params = prm; ix->n_contigs = n_contigs;
        ix->contig_off.assign(h_contig_off, h_contig_off + n_contigs + 1);
        const hipStream_t st = nullptr;
        KernelClock kc;
        EventPair untimed;      // (an index reports no kernel times of its own: the KernelClock's accounting alone)
        DBuf d_seq, d_cnt, d_scan;
        if (int rc = upload_pageable(d_seq, h_contig_seq, (size_t)total, 0, MAP_SLACK)) return rc;
        if (int rc = upload_pageable(ix->d_contig_off, h_contig_off, ((size_t)n_contigs + 1) * 8, 0, MAP_SLACK)) return rc;
        MapMinimizersDev mz;
        int64_t mz_bytes = total;
        if (int rc = timed_launch(kc, untimed, st, mz_bytes, [&] {
                const int rc = mz.run(d_seq.as<uint8_t>(), ix->d_contig_off.as<int64_t>(), n_contigs, total, prm, st);
                mz_bytes += 12 * mz.n;
                return rc; })) return rc;
        const int64_t n = ix->n_entries = mz.n;
        if (n > 0x7fffffff - HS_SCAN_TILE) { set_error("hs_map_index_create: more than 2^31 contig minimizers"); return HS_EINVAL; }
        ix->bucket_bits = hs::map_bucket_bits(prm, n);
        const int64_t n_buckets = (int64_t)1 << ix->bucket_bits;
        const uint32_t mask = (uint32_t)(n_buckets - 1);
        if (int rc = d_cnt.alloc((size_t)n_buckets * 4)) return rc;
        if (int rc = ix->d_bucket_off.alloc(((size_t)n_buckets + 1) * 8)) return rc;
        for (DBuf* b : {&ix->d_e_h, &ix->d_e_c, &ix->d_e_ts}) if (int rc = b->alloc((size_t)std::max<int64_t>(n, 1) * 4)) return rc;
        if (int rc = timed_launch(kc, untimed, st, 24 * n + 16 * n_buckets, [&]() -> int {
                HS_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)n_buckets * 4, st));
                const unsigned grid = (unsigned)((n + 255) / 256);
                if (n > 0) hipLaunchKernelGGL(hsdev::k_map_bucket_count, dim3(grid), dim3(256), 0, st, mz.h.as<uint32_t>(), (long long)n, mask, d_cnt.as<int32_t>());
                if (int rc = exclusive_scan_launch(d_cnt.as<int32_t>(), (int)n_buckets, ix->d_bucket_off.as<int64_t>(), d_scan, st)) return rc;
                HS_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)n_buckets * 4, st));
                if (n > 0) hipLaunchKernelGGL(hsdev::k_map_bucket_fill, dim3(grid), dim3(256), 0, st, mz.h.as<uint32_t>(), mz.ps.as<uint32_t>(), mz.seq.as<int32_t>(), (long long)n, mask,
                                              ix->d_bucket_off.as<int64_t>(), d_cnt.as<int32_t>(), ix->d_e_h.as<uint32_t>(), ix->d_e_c.as<int32_t>(), ix->d_e_ts.as<uint32_t>());
                HS_HIP(hipGetLastError());
                return HS_OK; })) return rc;
        if (int rc = stream_wait(st)) return rc;      // (the scratch goes back to the pool with this scope)
        kc.flush();
        *index = ix.release();
        return HS_OK;
    } catch (const std::exception& e) { set_error(std::string("hs_map_index_create: ") + e.what()); return HS_EINVAL; }
}

int hs_map_index_download(const hs_map_index* index, int64_t* n_entries, int32_t* bucket_bits, int64_t* bucket_off, uint32_t* e_hash, int32_t* e_contig, uint32_t* e_ts) {
    if (int rc = require_device()) return rc;
    if (!index) { set_error("hs_map_index_download: null argument"); return HS_EINVAL; }
    if (n_entries) *n_entries = index->n_entries;
    if (bucket_bits) *bucket_bits = index->bucket_bits;
    const hipStream_t st = nullptr;
    const size_t n = (size_t)index->n_entries;
    if (bucket_off) { if (int rc = d2h_pinned(bucket_off, index->d_bucket_off.p, (((size_t)1 << index->bucket_bits) + 1) * 8, st)) return rc; }
    if (e_hash && n) { if (int rc = d2h_pinned(e_hash, index->d_e_h.p, n * 4, st)) return rc; }
    if (e_contig && n) { if (int rc = d2h_pinned(e_contig, index->d_e_c.p, n * 4, st)) return rc; }
    if (e_ts && n) { if (int rc = d2h_pinned(e_ts, index->d_e_ts.p, n * 4, st)) return rc; }
    return HS_OK;
}

// The three map entries, each the stages of a MapCall it uses. Either way three waits: segments and anchors leave in the same shipment as the per-read block.
int hs_map_reads(const hs_map_index* index, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads, hs_map_result** result) {
    MapCall c("hs_map_reads", index, h_read_seq, h_read_off, n_reads);
    if (int rc = c.check(result != nullptr)) return rc;
    *result = nullptr;
    return c.run([&]() -> int {
        if (int rc = c.begin()) return rc;
        if (int rc = c.hits()) return rc;
        if (int rc = c.vote()) return rc;
        if (int rc = c.ship()) return rc;
        return c.make_result(result);
    });
}

int hs_map_reads_split(const hs_map_index* index, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads, const hs_map_split_params* split, hs_map_segments** segments) {
    const hs_map_split_params sp = split ? *split : hs_map_split_params_default();
    MapCall c("hs_map_reads_split", index, h_read_seq, h_read_off, n_reads);
    c.split = &sp;
    if (int rc = c.check(segments != nullptr)) return rc;
    *segments = nullptr;
    return c.run([&]() -> int {
        if (int rc = c.begin()) return rc;
        if (int rc = c.hits()) return rc;
        if (int rc = c.vote_split()) return rc;
        if (int rc = c.ship()) return rc;
        return c.make_segments(segments);
    });
}

int hs_map_reads_anchored(const hs_map_index* index, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads, const hs_map_anchor_params* params, hs_map_result** result,
                          hs_map_anchors** anchors) {
    const hs_map_anchor_params ap = params ? *params : hs_map_anchor_params_default();
    MapCall c("hs_map_reads_anchored", index, h_read_seq, h_read_off, n_reads);
    c.anchor = &ap;
    if (int rc = c.check(result && anchors)) return rc;
    *result = nullptr; *anchors = nullptr;
    return c.run([&]() -> int {
        if (int rc = c.begin()) return rc;
        if (int rc = c.hits()) return rc;
        if (int rc = c.vote()) return rc;
        if (int rc = c.anchors()) return rc;
        if (int rc = c.ship()) return rc;
        if (int rc = c.make_result(result)) return rc;
        const int rc = c.make_anchors(anchors);
        if (rc) { hs_map_result_destroy(*result); *result = nullptr; }
        return rc;
    });
}

// The three *_to_batch entries: a map call, its output as intervals, ToBatch::realign.
int hs_map_to_batch(const hs_map_index* index, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off,
                    int32_t n_reads, int32_t pad, hs_cv_batch** batch, hs_realign_records** records, hs_map_result** result) {
    const ToBatch to{h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, pad, batch, records, result, nullptr, nullptr};
    if (int rc = to.check("hs_map_to_batch", index)) return rc;
    MapOwned got;
    if (int rc = hs_map_reads(index, h_read_seq, h_read_off, n_reads, &got.result)) return rc;
    try { return to.realign(MappedIntervals(got.result, nullptr), false, got); }
    catch (const std::exception& e) { set_error(std::string("hs_map_to_batch: ") + e.what()); return HS_EINVAL; }
}

int hs_map_to_batch_anchored(const hs_map_index* index, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off,
                             int32_t n_reads, int32_t pad, const hs_map_anchor_params* params, hs_cv_batch** batch, hs_realign_records** records, hs_map_result** result,
                             hs_map_anchors** anchors) {
    const ToBatch to{h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, pad, batch, records, result, nullptr, anchors};
    if (int rc = to.check("hs_map_to_batch_anchored", index)) return rc;
    MapOwned got;
    if (int rc = hs_map_reads_anchored(index, h_read_seq, h_read_off, n_reads, params, &got.result, &got.anchors)) return rc;
    try { return to.realign(MappedIntervals(got.result, got.anchors), true, got); }
    catch (const std::exception& e) { set_error(std::string("hs_map_to_batch_anchored: ") + e.what()); return HS_EINVAL; }
}

int hs_map_split_to_batch(const hs_map_index* index, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off,
                          int32_t n_reads, int32_t pad, const hs_map_split_params* split, hs_cv_batch** batch, hs_realign_records** records, hs_map_segments** segments) {
    const ToBatch to{h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, pad, batch, records, nullptr, segments, nullptr};
    if (int rc = to.check("hs_map_split_to_batch", index)) return rc;
    MapOwned got;
    if (int rc = hs_map_reads_split(index, h_read_seq, h_read_off, n_reads, split, &got.segments)) return rc;
    const hs_map_segments* sg = got.segments;
    if (sg->n_segments > 0x7fffffff) { set_error("hs_map_split_to_batch: more than 2^31 segments in one call: map the reads in several calls"); return HS_EINVAL; }
    return to.realign(sg->read, sg->contig, sg->strand, sg->qstart, sg->qend, sg->tstart, sg->tend, sg->n_segments, nullptr, nullptr, nullptr, got);
}


// HS_MAP_SPLIT=<n>, n 2..8: hs_map_files writes the segment lines of hs_map_reads_split with max_segments = n. Unset, empty or 1: 0, the plain lines;
// anything else: the plain lines too, and a line on stderr that says so
static int map_split_from_env() {
    const char* e = std::getenv("HS_MAP_SPLIT");
    if (!e || !e[0] || (e[0] == '1' && !e[1])) return 0;
    if (!e[1] && e[0] >= '2' && e[0] <= '8') return e[0] - '0';
    std::fprintf(stderr, "hs_map: HS_MAP_SPLIT=%s is not one of 1..8: ignored, one line per mapped read is written\n", e);
    return 0;
}

// the job's files -> PAF lines of the mapped reads (HS_MAP_SPLIT: of their segments). An assembly that holds no S line and begins with '>' is read as FASTA.
int hs_map_files(const char* gfa, const char* reads, const char* out_paf, int32_t n_threads, const hs_map_params* params) {
    if (int rc = require_device()) return rc;
    if (!gfa || !reads || !out_paf) { set_error("hs_map_files: null argument"); return HS_EINVAL; }
    try {
        if (n_threads < 1) n_threads = host_threads();
        hs::SeqSet seqs;
        if (int rc = hs::load_sequences(gfa, reads, seqs, n_threads)) return rc;
        if (seqs.contig_names.empty()) hs::load_fasta_contigs(gfa, seqs);
        if (seqs.read_names.size() > 0x7fffffffu || seqs.contig_names.size() > 0x7fffffffu) { set_error("hs_map_files: more than 2^31 reads or contigs"); return HS_EINVAL; }
        const int32_t C = (int32_t)seqs.contig_names.size(), R = (int32_t)seqs.read_names.size();
        hs_map_index* ix = nullptr;
        if (int rc = hs_map_index_create(seqs.contig_seq.data(), seqs.contig_off.data(), C, params, &ix)) return rc;
        std::vector<const char*> rn((size_t)R), cn((size_t)C);
        for (int32_t i = 0; i < R; ++i) rn[(size_t)i] = seqs.read_names[(size_t)i].c_str();
        for (int32_t i = 0; i < C; ++i) cn[(size_t)i] = seqs.contig_names[(size_t)i].c_str();
        const bool timing = std::getenv("HS_TIMING") != nullptr;
        char* text = nullptr;
        int rc_text = HS_OK;
        if (const int n_split = map_split_from_env()) {
            hs_map_split_params sp = hs_map_split_params_default();
            sp.max_segments = n_split;
            hs_map_segments* sg = nullptr;
            const int rc = hs_map_reads_split(ix, seqs.read_seq.data(), seqs.read_off.data(), R, &sp, &sg);
            hs_map_index_destroy(ix);
            if (rc) return rc;
            rc_text = hs_map_segments_text(sg, rn.data(), seqs.read_off.data(), cn.data(), seqs.contig_off.data(), C, &text);
            int64_t n_mapped = 0, n_multi = 0;
            for (int32_t i = 0; i < R; ++i) { n_mapped += sg->seg_off[i + 1] > sg->seg_off[i]; n_multi += sg->seg_off[i + 1] - sg->seg_off[i] > 1; }
            if (timing) std::fprintf(stderr, "[hs timing] map: %ld of %d reads mapped, %ld of them in more than one segment (%ld segments), %ld minimizers, %ld hits, %ld reads through the scratch route, kernels %.2f + %.2f + %.2f ms\n",
                                     (long)n_mapped, R, (long)n_multi, (long)sg->n_segments, (long)sg->total_minimizers, (long)sg->total_hits, (long)sg->n_wide, sg->t_minimizers_ms, sg->t_hits_ms,
                                     sg->t_vote_ms);
            hs_map_segments_destroy(sg);
        } else {
            hs_map_result* res = nullptr;
            const int rc = hs_map_reads(ix, seqs.read_seq.data(), seqs.read_off.data(), R, &res);
            hs_map_index_destroy(ix);
            if (rc) return rc;
            rc_text = hs_map_text(res, rn.data(), seqs.read_off.data(), cn.data(), seqs.contig_off.data(), C, &text);
            int64_t n_mapped = 0;
            for (int32_t i = 0; i < R; ++i) n_mapped += res->contig[i] >= 0;
            if (timing) std::fprintf(stderr, "[hs timing] map: %ld of %d reads mapped, %ld minimizers, %ld hits, %ld reads through the scratch route, kernels %.2f + %.2f + %.2f ms\n",
                                     (long)n_mapped, R, (long)res->total_minimizers, (long)res->total_hits, (long)res->n_wide, res->t_minimizers_ms, res->t_hits_ms, res->t_vote_ms);
            hs_map_result_destroy(res);
        }
        if (rc_text) { set_error("hs_map_files: out of memory"); return rc_text; }
        std::ofstream o(out_paf);
        o << text;
        std::free(text);
        o.close();
        if (!o) { set_error(std::string("hs_map_files: could not write ") + out_paf); return HS_EIO; }
        return HS_OK;
    } catch (const std::exception& e) { set_error(std::string("hs_map_files: ") + e.what()); return HS_EINVAL; }
}

// argv = <gfa|fasta> <reads> <out.paf> [threads]
int hs_map_main(int argc, char** argv) {
    if (argc < 4) { std::cout << "Usage: hs_map <gfa|fasta> <reads> <out.paf> [threads]\n"; return argc < 2 ? 0 : 1; }
    const int threads = argc > 4 ? std::atoi(argv[4]) : 0;
    if (int rc = hs_map_files(argv[1], argv[2], argv[3], threads, nullptr)) {
        std::cout << "ERROR: " << hs_last_error() << " (" << rc << ")" << std::endl;
        return 1;
    }
    return 0;
}

}  // extern "C"
