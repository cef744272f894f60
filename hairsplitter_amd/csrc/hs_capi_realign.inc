// hs_capi_realign.inc -- part of hs_capi.hip: the CIGAR-less input without the files in between. Intervals in memory (or the PAF
// lines of hs_realign.cpp's parser) -> pairs cut on the device (k_realign_cut) -> A1 (hs_edlib_hw_align) -> CIGAR words on the
// device (k_m2c_count, the scan, k_m2c_write; hs_kernels_realign.hip) -> the records in the layout of hs_cv_batch_create and the
// batch made from them. Per round only the words, positions, distances and lengths come back to the host.
// hs_realign_intervals and hs_realign_intervals_anchored are one job (realign_job): the second cuts every interval at given anchors first, pieces per
// class -> k_realign_cut -> at most three aligner calls; a round that holds a cut interval joins its pieces (k_anchor_join_plan / k_anchor_join) before
// the same words, positions and download, a round that holds none takes the aligner's output as it is.
namespace {

// The three launches of hs_moves_to_cigar with their scratch: count() leaves offsets, total and spans, write() lays the words down.
struct MovesToCigar {
    DBuf d_ops_off, d_chunk_first, d_cnt, d_start, d_woff, d_scan;
    UploadPack pk;
    std::vector<int64_t> ops_off;
    std::vector<int32_t> chunk_first;
    int32_t n = 0, n_chunks = 0;
    const uint8_t* d_ops = nullptr; const int32_t* d_ops_len = nullptr; const int32_t* d_clip_left = nullptr; const int32_t* d_clip_right = nullptr;

    int count(const uint8_t* ops, const int64_t* h_ops_off, const int32_t* ops_len, const int32_t* clip_left, const int32_t* clip_right, int32_t n_pairs,
              int64_t* d_word_off, int32_t* d_spans, int64_t* n_words, hipStream_t stream) {
        n = n_pairs; d_ops = ops; d_ops_len = ops_len; d_clip_left = clip_left; d_clip_right = clip_right;
        ops_off.assign(h_ops_off, h_ops_off + n + 1);
        chunk_first.assign((size_t)n + 1, 0);
        int64_t chunks = 0;
        for (int32_t i = 0; i < n; ++i) {
            const int64_t room = ops_off[(size_t)i + 1] - ops_off[(size_t)i];
            if (room < 0 || room >= ((int64_t)1 << 28)) { set_error("hs_moves_to_cigar: pair " + std::to_string(i) + " has room for " + std::to_string(room) + " moves (0 .. 2^28 - 1: the length field of a CIGAR word)"); return HS_EINVAL; }
            chunks += (room + hsdev::M2C_CHUNK - 1) / hsdev::M2C_CHUNK;
            if (chunks > 0x7fffffff - 4) { set_error("hs_moves_to_cigar: more than 2^31 chunks of moves in one call"); return HS_EINVAL; }
            chunk_first[(size_t)i + 1] = (int32_t)chunks;
        }
        n_chunks = (int32_t)chunks;
        if (d_spans) HS_HIP(hipMemsetAsync(d_spans, 0, sizeof(int32_t) * 2 * (size_t)n, stream));
        if (n_chunks == 0) {
            HS_HIP(hipMemsetAsync(d_word_off, 0, sizeof(int64_t) * ((size_t)n + 1), stream));
            *n_words = 0;
            return stream_wait(stream);
        }
        pk.add(ops_off, d_ops_off); pk.add(chunk_first, d_chunk_first);
        if (int rc = pk.commit(stream)) return rc;
        if (int rc = d_cnt.alloc(sizeof(int32_t) * (size_t)n_chunks)) return rc;
        if (int rc = d_start.alloc(sizeof(int32_t) * (size_t)n_chunks)) return rc;
        if (int rc = d_woff.alloc(sizeof(int64_t) * ((size_t)n_chunks + 1))) return rc;
        hipLaunchKernelGGL(hsdev::k_m2c_count, dim3((unsigned)((n_chunks + 3) / 4)), dim3(256), 0, stream, d_ops, d_ops_off.as<int64_t>(), d_ops_len, d_clip_left, d_clip_right, n,
                           d_chunk_first.as<int32_t>(), n_chunks, d_cnt.as<int32_t>(), d_start.as<int32_t>(), d_spans);
        HS_HIP(hipGetLastError());
        if (int rc = exclusive_scan_launch(d_cnt.as<int32_t>(), n_chunks, d_woff.as<int64_t>(), d_scan, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_m2c_pair_off, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, stream, d_chunk_first.as<int32_t>(), n, d_woff.as<int64_t>(), d_word_off);
        HS_HIP(hipGetLastError());
        return copy_d2h(n_words, d_woff.as<int64_t>() + n_chunks, sizeof(int64_t), stream);
    }
    // (after count(); d_words has room for the total it returned)
    int write(uint32_t* d_words, hipStream_t stream) {
        if (n_chunks == 0) return HS_OK;
        hipLaunchKernelGGL(hsdev::k_m2c_write, dim3((unsigned)((n_chunks + 3) / 4)), dim3(256), 0, stream, d_ops, d_ops_off.as<int64_t>(), d_ops_len, d_clip_left, d_clip_right, n,
                           d_chunk_first.as<int32_t>(), n_chunks, d_start.as<int32_t>(), d_woff.as<int64_t>(), d_words);
        HS_HIP(hipGetLastError());
        return stream_wait(stream);
    }
};

// one of the two buffers hs_edlib_hw_align takes, cut from a resident sequence buffer: d_out has room for off[m] rounded up to 16
static int realign_cut_launch(const DBuf& d_off, const DBuf& d_src, const uint8_t* d_rev, int32_t m, int64_t total, const uint8_t* d_seq, uint8_t* d_out, hipStream_t stream) {
    if (m <= 0 || total <= 0) return HS_OK;
    const int64_t out_bytes = (total + 15) & ~(int64_t)15;
    hipLaunchKernelGGL(hsdev::k_realign_cut, dim3((unsigned)((out_bytes + 4095) >> 12)), dim3(256), 0, stream, d_off.as<int64_t>(), d_src.as<int64_t>(), d_rev, m, d_seq, d_out, out_bytes);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// the join of a round's pieces: the plan (a lane per interval), then the joined strings (a lane per 16-byte block of J.joined_bytes)
static int anchor_join_launch(const hsdev::AnchorJoinArgs& J, hipStream_t stream) {
    hipLaunchKernelGGL(hsdev::k_anchor_join_plan, dim3((unsigned)(J.m / 256 + 1)), dim3(256), 0, stream, J);
    if (J.joined_bytes > 0) hipLaunchKernelGGL(hsdev::k_anchor_join, dim3((unsigned)((J.joined_bytes + 4095) >> 12)), dim3(256), 0, stream, J);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// the checks of hs_realign.cpp's parser on every interval; the intervals of every contig, in input order
static int realign_check_intervals(const int64_t* h_contig_off, int32_t n_contigs, const int64_t* h_read_off, int32_t n_reads, const int32_t* iv_read, const int32_t* iv_contig,
                                   const int32_t* iv_qstart, const int32_t* iv_qend, const int32_t* iv_tstart, const int32_t* iv_tend, size_t n, std::vector<int32_t>& contig_iv_off,
                                   std::vector<int32_t>& order) {
    contig_iv_off.assign((size_t)n_contigs + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const bool ids = iv_read[i] >= 0 && iv_read[i] < n_reads && iv_contig[i] >= 0 && iv_contig[i] < n_contigs;
        const int64_t rl = ids ? h_read_off[iv_read[i] + 1] - h_read_off[iv_read[i]] : 0, cl = ids ? h_contig_off[iv_contig[i] + 1] - h_contig_off[iv_contig[i]] : 0;
        if (!ids || iv_qstart[i] < 0 || iv_qend[i] > rl || iv_qstart[i] >= iv_qend[i] || iv_tstart[i] < 0 || iv_tend[i] > cl || iv_tstart[i] >= iv_tend[i]) {
            set_error("hs_realign_intervals: interval " + std::to_string(i) + " (read " + std::to_string(iv_read[i]) + " [" + std::to_string(iv_qstart[i]) + ", " + std::to_string(iv_qend[i])
                      + "), contig " + std::to_string(iv_contig[i]) + " [" + std::to_string(iv_tstart[i]) + ", " + std::to_string(iv_tend[i]) + ")) does not fit its read / contig");
            return HS_EINVAL;
        }
        contig_iv_off[(size_t)iv_contig[i] + 1]++;
    }
    for (int c = 0; c < n_contigs; ++c) contig_iv_off[(size_t)c + 1] += contig_iv_off[(size_t)c];
    order.assign(n, 0);
    std::vector<int32_t> at(contig_iv_off.begin(), contig_iv_off.end() - 1);
    for (size_t i = 0; i < n; ++i) order[(size_t)at[(size_t)iv_contig[i]]++] = (int32_t)i;
    return HS_OK;
}

// what a job's rounds add up to, and the records made from them (contig_rec_off holds the counts per contig; `dropped` in any order): the one end of
// hs_realign_intervals and hs_realign_intervals_anchored
struct RealignTotals { double t_cut, t_align, t_cigar, t_download, t_join; int64_t n_rounds, move_bytes, n_pieces; };
static int realign_make_records(const char* who, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off,
                                int32_t n_reads, int32_t n_intervals, std::vector<int32_t>& rec_interval, std::vector<int32_t>& rec_read, std::vector<int32_t>& rec_pos,
                                std::vector<int32_t>& rec_dist, std::vector<int32_t>& contig_rec_off, std::vector<int32_t>& dropped, std::vector<uint8_t>& rec_strand,
                                std::vector<int64_t>& rec_cig_off, std::vector<uint32_t, hs::NoInitAlloc<uint32_t>>& cigar, const RealignTotals& tot, hs_realign_records** out,
                                hs_cv_batch** batch) {
    for (int c = 0; c < n_contigs; ++c) contig_rec_off[(size_t)c + 1] += contig_rec_off[(size_t)c];
    std::sort(dropped.begin(), dropped.end());
    if (!dropped.empty())
        std::fprintf(stderr, "hairsplitter: realign: %ld of %ld intervals have no alignment (the device aligner found none, or the read segment is longer than 2^20 bases) and were left out\n",
                     (long)dropped.size(), (long)n_intervals);
    hs_realign_records* r = (hs_realign_records*)std::calloc(1, sizeof(hs_realign_records));
    if (!r) { set_error(std::string(who) + ": out of memory"); return HS_EINVAL; }
    r->n_intervals = n_intervals; r->n_rec = (int32_t)rec_read.size(); r->n_contigs = n_contigs;
    r->contig_rec_off = malloc_copy(contig_rec_off); r->rec_interval = malloc_copy(rec_interval); r->rec_read = malloc_copy(rec_read); r->rec_pos = malloc_copy(rec_pos);
    r->rec_dist = malloc_copy(rec_dist); r->rec_strand = malloc_copy(rec_strand); r->rec_cig_off = malloc_copy(rec_cig_off);
    r->cigar = (uint32_t*)std::malloc(std::max<size_t>(1, cigar.size()) * sizeof(uint32_t));
    if (r->cigar && !cigar.empty()) std::memcpy(r->cigar, cigar.data(), cigar.size() * sizeof(uint32_t));
    r->n_dropped = (int64_t)dropped.size(); r->dropped = malloc_copy(dropped);
    r->t_cut_ms = tot.t_cut; r->t_align_ms = tot.t_align; r->t_cigar_ms = tot.t_cigar; r->t_download_ms = tot.t_download; r->t_join_ms = tot.t_join;
    r->n_rounds = tot.n_rounds; r->move_bytes = tot.move_bytes; r->cigar_words = (int64_t)cigar.size(); r->n_pieces = tot.n_pieces;
    if (!r->contig_rec_off || !r->rec_interval || !r->rec_read || !r->rec_pos || !r->rec_dist || !r->rec_strand || !r->rec_cig_off || !r->cigar || !r->dropped) {
        hs_realign_records_destroy(r); set_error(std::string(who) + ": out of memory"); return HS_EINVAL;
    }
    if (batch) {
        if (int rc = hs_cv_batch_create(h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, r->rec_read, r->rec_pos, r->rec_strand, r->rec_cig_off, r->cigar,
                                        r->contig_rec_off, batch)) { hs_realign_records_destroy(r); return rc; }
    }
    *out = r;
    return HS_OK;
}

}  // namespace

int hs_moves_to_cigar(const uint8_t* d_ops, const int64_t* h_ops_off, const int32_t* d_ops_len, const int32_t* d_clip_left, const int32_t* d_clip_right, int32_t n,
                      int64_t* d_word_off, uint32_t* d_words, int64_t words_cap, int32_t* d_spans, int64_t* n_words, void* stream) {
    if (int rc = require_device()) return rc;
    if (n < 0) { set_error("hs_moves_to_cigar: negative number of pairs"); return HS_EINVAL; }
    if (n == 0) {
        if (n_words) *n_words = 0;
        if (d_word_off) { HS_HIP(hipMemsetAsync(d_word_off, 0, sizeof(int64_t), (hipStream_t)stream)); return stream_wait((hipStream_t)stream); }
        return HS_OK;
    }
    if (!d_ops || !h_ops_off || !d_ops_len || !d_word_off || !n_words || (d_words && words_cap < 0)) { set_error("hs_moves_to_cigar: bad arguments"); return HS_EINVAL; }
    MovesToCigar mc;
    if (int rc = mc.count(d_ops, h_ops_off, d_ops_len, d_clip_left, d_clip_right, n, d_word_off, d_spans, n_words, (hipStream_t)stream)) return rc;
    if (!d_words) return HS_OK;
    if (words_cap < *n_words) { set_error("hs_moves_to_cigar: the pairs have " + std::to_string(*n_words) + " words, words_cap is " + std::to_string(words_cap)); return HS_EINVAL; }
    return mc.write(d_words, (hipStream_t)stream);      // (synchronous: the scratch goes back to the pool with this scope)
}

void hs_realign_records_destroy(hs_realign_records* r) {
    if (!r) return;
    void* p[] = {r->contig_rec_off, r->rec_interval, r->rec_read, r->rec_pos, r->rec_dist, r->rec_strand, r->rec_cig_off, r->cigar, r->dropped};
    for (void* q : p) std::free(q);
    std::free(r);
}

namespace {

// the pairs one class of pieces hands to its aligner call: offsets from 0, the cut's sources, where its results lie in the round's arrays
struct PieceClass {
    std::vector<int64_t> q_off{0}, t_off{0}, o_off{0}, q_src, t_src;
    std::vector<uint8_t> q_rev, t_rev;
    int64_t first = 0, ops_at = 0;      // its section of the numbers (an index) and of the moves (a byte offset)
    size_t size() const { return q_src.size(); }
    void add(int64_t qs, bool qr, int64_t ql, int64_t ts, bool tr, int64_t tl) {
        q_src.push_back(qs); q_rev.push_back(qr ? 1 : 0); t_src.push_back(ts); t_rev.push_back(tr ? 1 : 0);
        q_off.push_back(q_off.back() + ql); t_off.push_back(t_off.back() + tl); o_off.push_back(o_off.back() + ql + tl);
    }
};

// The one job behind hs_realign_intervals (anc_off NULL: no interval has anchors) and hs_realign_intervals_anchored: checks, uploads, rounds, records.
// Per round: every interval's pieces by class (include/hairsplitter_hip.h; hs_map_host.h, "anchors") -- an interval without anchors is one HW piece --,
// k_realign_cut per class and side (a head's two strings are cut backwards; complementing both keeps every equality), at most three aligner calls -- HW,
// SHW PATH for heads and tails, NW PATH for middles. A round whose intervals are all one HW piece is `direct`: the aligner's moves, lengths and
// distances are the intervals' own and k_realign_pos gives POS. Any other round joins its pieces first (k_anchor_join_plan, k_anchor_join). Then one
// tail: words on the device, the download, the records.
static int realign_job(const char* who, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off,
                       int32_t n_reads, const int32_t* iv_read, const int32_t* iv_contig, const uint8_t* iv_strand, const int32_t* iv_qstart, const int32_t* iv_qend,
                       const int32_t* iv_tstart, const int32_t* iv_tend, int32_t n_intervals, int32_t pad, const int64_t* anc_off, const int32_t* anc_q, const int32_t* anc_t,
                       hs_realign_records** out, hs_cv_batch** batch) {
    if (int rc = require_device()) return rc;
    if (!out || !h_contig_off || !h_read_off || n_contigs < 0 || n_reads < 0 || n_intervals < 0 || pad < 0
        || (n_intervals > 0 && (!iv_read || !iv_contig || !iv_strand || !iv_qstart || !iv_qend || !iv_tstart || !iv_tend))) {
        set_error(std::string(who) + ": bad arguments"); return HS_EINVAL;
    }
    *out = nullptr;
    if (batch) *batch = nullptr;
    try {
        const size_t n = (size_t)n_intervals;
        std::vector<int32_t> contig_iv_off, order;
        if (int rc = realign_check_intervals(h_contig_off, n_contigs, h_read_off, n_reads, iv_read, iv_contig, iv_qstart, iv_qend, iv_tstart, iv_tend, n, contig_iv_off, order)) return rc;
        // the contig window of an interval, and its read range as it aligns
        auto window = [&](size_t i, int& w0, int& w1) {
            w0 = std::max(0, iv_tstart[i] - pad);
            w1 = (int)std::min<int64_t>(h_contig_off[iv_contig[i] + 1] - h_contig_off[iv_contig[i]], (int64_t)iv_tend[i] + pad);
        };
        auto range = [&](size_t i, int& a0, int& a1) {
            const int Lr = (int)(h_read_off[iv_read[i] + 1] - h_read_off[iv_read[i]]);
            a0 = iv_strand[i] ? iv_qstart[i] : Lr - iv_qend[i]; a1 = iv_strand[i] ? iv_qend[i] : Lr - iv_qstart[i];
        };
        auto n_anchors = [&](size_t i) { return anc_off ? anc_off[i + 1] - anc_off[i] : (int64_t)0; };
        if (anc_off) {
            bool offsets_ok = anc_off[0] == 0;
            for (size_t i = 0; offsets_ok && i < n; ++i) offsets_ok = anc_off[i + 1] >= anc_off[i] && anc_off[i + 1] - anc_off[i] <= 0x7fffffff;
            if (!offsets_ok || (anc_off[n] > 0 && (!anc_q || !anc_t))) { set_error(std::string(who) + ": anc_off must ascend from 0, and anc_q / anc_t hold anc_off[n_intervals] anchors"); return HS_EINVAL; }
            for (size_t i = 0; i < n; ++i) {
                int a0, a1; range(i, a0, a1);
                for (int64_t j = anc_off[i]; j < anc_off[i + 1]; ++j) {
                    const bool rises = j == anc_off[i] || (anc_q[j] > anc_q[j - 1] && anc_t[j] > anc_t[j - 1]);
                    if (!rises || anc_q[j] < a0 || anc_q[j] > a1 || anc_t[j] < iv_tstart[i] || anc_t[j] > iv_tend[i]) {
                        set_error(std::string(who) + ": interval " + std::to_string(i) + ": anchor " + std::to_string(j - anc_off[i]) + " (q " + std::to_string(anc_q[j]) + ", t "
                                  + std::to_string(anc_t[j]) + ") does not ascend strictly in q and t or lies outside the interval (read as it aligns [" + std::to_string(a0) + ", " + std::to_string(a1)
                                  + "], contig [" + std::to_string(iv_tstart[i]) + ", " + std::to_string(iv_tend[i]) + "])");
                        return HS_EINVAL;
                    }
                }
            }
        }
        const hipStream_t stream = nullptr;
        DBuf d_contigs, d_reads;      // the job's first device copy of the sequences: back in the pool before the batch is made
        if (n) {
            if (int rc = upload_pageable(d_contigs, h_contig_seq, (size_t)h_contig_off[n_contigs], HS_SEQ_PAD, HS_SEQ_PAD)) return rc;
            if (int rc = upload_pageable(d_reads, h_read_seq, (size_t)h_read_off[n_reads], HS_SEQ_PAD, HS_SEQ_PAD)) return rc;
        }
        std::vector<int32_t> rec_interval, rec_read, rec_pos, rec_dist, contig_rec_off((size_t)n_contigs + 1, 0), dropped;
        std::vector<uint8_t> rec_strand;
        std::vector<int64_t> rec_cig_off(1, 0);
        std::vector<uint32_t, hs::NoInitAlloc<uint32_t>> cigar;
        RealignTotals tot{};
        auto wall = [] { return std::chrono::steady_clock::now(); };
        auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        const size_t chunk_bases = hs::realign_chunk_bases();
        size_t done = 0;
        while (done < n) {
            // ---- the intervals of a round, bounded as in hs_realign.cpp: an interval needs query + window bases and as many move bytes; its pieces
            // stay together and count as pairs ----
            size_t k1 = done, bases = 0, pairs = 0;
            while (k1 < n && (k1 == done || (bases < chunk_bases && pairs + (size_t)n_anchors((size_t)order[k1]) + 1 <= 1000000))) {
                const size_t i = (size_t)order[k1];
                int w0, w1; window(i, w0, w1);
                bases += (size_t)(iv_qend[i] - iv_qstart[i]) + (size_t)(w1 - w0);
                pairs += (size_t)n_anchors(i) + 1;
                ++k1;
            }
            const size_t m = k1 - done;
            // ---- the piece table: what the host needs for the launches follows from the interval lengths and the anchors alone ----
            PieceClass cls[3];      // 0: HW, 1: SHW (heads and tails), 2: NW
            std::vector<int32_t> iv_piece(m + 1, 0), iv_base(m), clip_l(m), clip_r(m), pc_idx, pc_room;
            std::vector<int64_t> join_off(m + 1, 0), pc_ops;
            std::vector<uint8_t> pc_kind, pc_cls;
            for (size_t k = 0; k < m; ++k) {
                const size_t i = (size_t)order[done + k];
                int w0, w1, a0, a1; window(i, w0, w1); range(i, a0, a1);
                const int qlen = (int)(h_read_off[iv_read[i] + 1] - h_read_off[iv_read[i]]);
                const bool minus = iv_strand[i] == 0;
                const int64_t rbase = h_read_off[iv_read[i]], cbase = h_contig_off[iv_contig[i]];
                clip_l[k] = a0; clip_r[k] = qlen - a1;
                join_off[k + 1] = join_off[k] + (a1 - a0) + (w1 - w0);
                // the read bases [x0, x1) as they align, forwards (or backwards, for a head), against the contig bases [t0, t1)
                auto piece = [&](int c, int kind, int x0, int x1, int t0, int t1) {
                    const bool back = kind == hsdev::ANCHOR_HEAD;
                    const int64_t qs = rbase + (minus ? (back ? qlen - x1 : qlen - 1 - x0) : (back ? x1 - 1 : x0));
                    cls[c].add(qs, minus != back, x1 - x0, cbase + (back ? t1 - 1 : t0), back, t1 - t0);
                    pc_kind.push_back((uint8_t)kind); pc_cls.push_back((uint8_t)c); pc_idx.push_back((int32_t)cls[c].size() - 1); pc_room.push_back((x1 - x0) + (t1 - t0));
                };
                auto insertions = [&](int count) { pc_kind.push_back((uint8_t)hsdev::ANCHOR_INS); pc_cls.push_back(3); pc_idx.push_back(count); pc_room.push_back(count); };
                if (n_anchors(i) == 0) { iv_base[k] = w0; piece(0, hsdev::ANCHOR_HW, a0, a1, w0, w1); }
                else {
                    const int64_t j0 = anc_off[i], j1 = anc_off[i + 1];
                    iv_base[k] = anc_t[j0];
                    if (anc_q[j0] > a0) { if (anc_t[j0] > w0) piece(1, hsdev::ANCHOR_HEAD, a0, anc_q[j0], w0, anc_t[j0]); else insertions(anc_q[j0] - a0); }
                    for (int64_t j = j0; j + 1 < j1; ++j) piece(2, hsdev::ANCHOR_MID, anc_q[j], anc_q[j + 1], anc_t[j], anc_t[j + 1]);
                    if (anc_q[j1 - 1] < a1) { if (anc_t[j1 - 1] < w1) piece(1, hsdev::ANCHOR_TAIL, anc_q[j1 - 1], a1, anc_t[j1 - 1], w1); else insertions(a1 - anc_q[j1 - 1]); }
                }
                iv_piece[k + 1] = (int32_t)pc_kind.size();
            }
            const bool direct = cls[0].size() == m;      // (every interval of the round is one HW piece: class 0's pair k is interval k)
            const int n_cls = direct ? 1 : 3;
            // the classes' sections: numbers from a multiple of 64, moves from a multiple of 256
            int64_t n_num = 0, n_ops = 0;
            for (PieceClass& c : cls) { c.first = n_num; c.ops_at = n_ops; n_num = (n_num + (int64_t)c.size() + 63) & ~(int64_t)63; n_ops = (n_ops + c.o_off.back() + 16 + 255) & ~(int64_t)255; }
            const size_t P = pc_kind.size();
            tot.n_pieces += (int64_t)(cls[0].size() + cls[1].size() + cls[2].size());
            DBuf d_q_off[3], d_t_off[3], d_q_src[3], d_t_src[3], d_q_rev[3], d_t_rev[3], d_q[3], d_t[3];
            DBuf d_iv_piece, d_iv_base, d_clip_l, d_clip_r, d_join_off, d_pc_idx, d_pc_room, d_pc_ops, d_pc_kind, dd, ds, de, dlen, dops, d_pc_at, d_len, d_dist, d_pos, d_joined, d_word_off, d_words;
            UploadPack pk;
            for (int c = 0; c < n_cls; ++c) {
                pk.add(cls[c].q_off, d_q_off[c]); pk.add(cls[c].t_off, d_t_off[c]); pk.add(cls[c].q_src, d_q_src[c]); pk.add(cls[c].t_src, d_t_src[c]); pk.add(cls[c].q_rev, d_q_rev[c]);
                if (c > 0) pk.add(cls[c].t_rev, d_t_rev[c]);      // (an HW piece's window is never cut backwards: no flags)
            }
            pk.add(iv_base, d_iv_base); pk.add(clip_l, d_clip_l); pk.add(clip_r, d_clip_r);
            if (!direct) {      // the join's table
                pc_ops.assign(P, 0);
                for (size_t p = 0; p < P; ++p) {
                    if (pc_cls[p] > 2) continue;
                    const PieceClass& c = cls[pc_cls[p]];
                    pc_ops[p] = c.ops_at + c.o_off[(size_t)pc_idx[p]];
                    pc_idx[p] = (int32_t)(c.first + pc_idx[p]);
                }
                pk.add(iv_piece, d_iv_piece); pk.add(join_off, d_join_off); pk.add(pc_idx, d_pc_idx); pk.add(pc_room, d_pc_room); pk.add(pc_ops, d_pc_ops); pk.add(pc_kind, d_pc_kind);
            }
            if (int rc = pk.commit(stream)) return rc;
            for (int c = 0; c < n_cls; ++c) {
                if (int rc = d_q[c].alloc((size_t)cls[c].q_off.back() + 16)) return rc;
                if (int rc = d_t[c].alloc((size_t)cls[c].t_off.back() + 16)) return rc;
            }
            if (int rc = dops.alloc((size_t)(direct ? cls[0].o_off.back() : n_ops) + 16)) return rc;
            for (DBuf* b : {&dd, &ds, &de, &dlen}) if (int rc = b->alloc((direct ? m : (size_t)std::max<int64_t>(n_num, 64)) * sizeof(int32_t))) return rc;
            if (int rc = d_pos.alloc(m * sizeof(int32_t))) return rc;
            if (int rc = d_word_off.alloc((m + 1) * sizeof(int64_t))) return rc;
            const int64_t joined_bytes = (join_off[m] + 15) & ~(int64_t)15;
            if (!direct) {
                if (int rc = d_pc_at.alloc(std::max<size_t>(P, 1) * sizeof(int32_t))) return rc;
                for (DBuf* b : {&d_len, &d_dist}) if (int rc = b->alloc(m * sizeof(int32_t))) return rc;
                if (int rc = d_joined.alloc((size_t)joined_bytes + 16)) return rc;
            }
            // ---- cut: each class's two buffers ----
            EventPair ev_cut, ev_join;      // (whatever the step: the records report the cut's and the join's time of every call)
            if (int rc = ev_cut.take()) return rc;
            if (!direct) { if (int rc = ev_join.take()) return rc; }
            HS_HIP(ev_rec(ev_cut.a, stream));
            for (int c = 0; c < n_cls; ++c) {
                const int32_t mc = (int32_t)cls[c].size();
                if (int rc = realign_cut_launch(d_q_off[c], d_q_src[c], d_q_rev[c].as<uint8_t>(), mc, cls[c].q_off.back(), d_reads.as<uint8_t>() + HS_SEQ_PAD, d_q[c].as<uint8_t>(), stream)) return rc;
                if (int rc = realign_cut_launch(d_t_off[c], d_t_src[c], d_t_rev[c].as<uint8_t>(), mc, cls[c].t_off.back(), d_contigs.as<uint8_t>() + HS_SEQ_PAD, d_t[c].as<uint8_t>(), stream)) return rc;
            }
            HS_HIP(ev_rec(ev_cut.b, stream));
            // ---- align (synchronous): at most three calls, none for a class without pieces ----
            auto t0 = wall();
            bool aligned = false;
            for (int c = 0; c < n_cls; ++c) {
                const int32_t mc = (int32_t)cls[c].size();
                if (mc == 0) continue;
                int32_t* dist = dd.as<int32_t>() + cls[c].first; int32_t* start = ds.as<int32_t>() + cls[c].first; int32_t* end = de.as<int32_t>() + cls[c].first;
                int32_t* len = dlen.as<int32_t>() + cls[c].first;
                uint8_t* ops = dops.as<uint8_t>() + cls[c].ops_at;
                const int rc = c == 0 ? hs_edlib_hw_align(d_q[c].as<uint8_t>(), cls[c].q_off.data(), d_t[c].as<uint8_t>(), cls[c].t_off.data(), mc, dist, start, end, ops, cls[c].o_off.data(), len, stream)
                                      : hs_edlib_align(d_q[c].as<uint8_t>(), cls[c].q_off.data(), d_t[c].as<uint8_t>(), cls[c].t_off.data(), mc, c == 1 ? 1 : 0, 2, -1, dist, start, end, nullptr, ops,
                                                       cls[c].o_off.data(), len, stream);
                if (rc) return rc;
                aligned = true;
            }
            if (!aligned) { if (int rc = stream_wait(stream)) return rc; }      // (a round without an aligner call: the cut's events)
            float cut_ms = 0, join_ms = 0;
            if (int rc = ev_cut.ms(&cut_ms)) return rc;
            tot.t_cut += cut_ms; tot.t_align += ms_since(t0) - cut_ms;      // (the cut runs ahead of the aligner on the same stream)
            // ---- join: every interval's piece moves as one string; a direct round's are the aligner's ----
            t0 = wall();
            const uint8_t* r_ops = dops.as<uint8_t>();
            const int64_t* r_ops_off = cls[0].o_off.data();
            const int32_t* r_len = dlen.as<int32_t>(); const int32_t* r_dist = dd.as<int32_t>();
            if (!direct) {
                hsdev::AnchorJoinArgs J{};
                J.m = (int)m; J.iv_piece = d_iv_piece.as<int32_t>(); J.iv_base = d_iv_base.as<int32_t>(); J.join_off = d_join_off.as<int64_t>();
                J.pc_kind = d_pc_kind.as<uint8_t>(); J.pc_idx = d_pc_idx.as<int32_t>(); J.pc_room = d_pc_room.as<int32_t>(); J.pc_ops = d_pc_ops.as<int64_t>();
                J.ops = dops.as<uint8_t>(); J.dist = dd.as<int32_t>(); J.start = ds.as<int32_t>(); J.end = de.as<int32_t>(); J.len = dlen.as<int32_t>();
                J.pc_at = d_pc_at.as<int32_t>(); J.out_len = d_len.as<int32_t>(); J.out_dist = d_dist.as<int32_t>(); J.out_pos = d_pos.as<int32_t>();
                J.joined = d_joined.as<uint8_t>(); J.joined_bytes = joined_bytes;
                HS_HIP(ev_rec(ev_join.a, stream));
                if (int rc = anchor_join_launch(J, stream)) return rc;
                HS_HIP(ev_rec(ev_join.b, stream));
                r_ops = d_joined.as<uint8_t>(); r_ops_off = join_off.data(); r_len = d_len.as<int32_t>(); r_dist = d_dist.as<int32_t>();
            }
            // ---- moves -> words: an interval without a path gets none, so the words of the round lie compact ----
            MovesToCigar mc;
            int64_t n_words = 0;
            if (int rc = mc.count(r_ops, r_ops_off, r_len, d_clip_l.as<int32_t>(), d_clip_r.as<int32_t>(), (int32_t)m, d_word_off.as<int64_t>(), nullptr, &n_words, stream)) return rc;
            if (int rc = d_words.alloc(std::max<size_t>(1, (size_t)n_words) * sizeof(uint32_t))) return rc;
            if (direct) {
                hipLaunchKernelGGL(hsdev::k_realign_pos, dim3((unsigned)(m / 256 + 1)), dim3(256), 0, stream, d_iv_base.as<int32_t>(), ds.as<int32_t>(), (int)m, d_pos.as<int32_t>());
                HS_HIP(hipGetLastError());
            }
            if (int rc = mc.write(d_words.as<uint32_t>(), stream)) return rc;
            if (int rc = ev_join.ms(&join_ms)) return rc;      // (0 for a direct round: it took no events)
            tot.t_join += join_ms; tot.t_cigar += ms_since(t0) - join_ms;
            // ---- words, positions, distances, lengths ----
            t0 = wall();
            std::vector<int32_t> pos(m), dist(m), olen(m);
            std::vector<int64_t> word_off(m + 1);
            const size_t w_at = cigar.size();
            cigar.resize(w_at + (size_t)n_words);
            if (int rc = d2h_pinned(cigar.data() + w_at, d_words.p, (size_t)n_words * sizeof(uint32_t), stream)) return rc;
            if (int rc = d2h_pinned(word_off.data(), d_word_off.p, (m + 1) * sizeof(int64_t), stream)) return rc;
            if (int rc = d2h_pinned(pos.data(), d_pos.p, m * sizeof(int32_t), stream)) return rc;
            if (int rc = d2h_pinned(dist.data(), r_dist, m * sizeof(int32_t), stream)) return rc;
            if (int rc = d2h_pinned(olen.data(), r_len, m * sizeof(int32_t), stream)) return rc;
            tot.t_download += ms_since(t0);
            for (size_t k = 0; k < m; ++k) {
                const size_t i = (size_t)order[done + k];
                if (olen[k] <= 0) { dropped.push_back((int32_t)i); continue; }      // (edlib has no alignment for this interval: no record)
                rec_interval.push_back((int32_t)i); rec_read.push_back(iv_read[i]); rec_pos.push_back(pos[k]); rec_dist.push_back(dist[k]);
                rec_strand.push_back(iv_strand[i] ? 1 : 0);
                rec_cig_off.push_back((int64_t)w_at + word_off[k + 1]);
                contig_rec_off[(size_t)iv_contig[i] + 1]++;
                tot.move_bytes += olen[k];
            }
            ++tot.n_rounds;
            done = k1;
        }
        d_contigs.release(); d_reads.release();      // (the pool hands the same blocks to hs_cv_batch_create below)
        return realign_make_records(who, h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, n_intervals, rec_interval, rec_read, rec_pos, rec_dist,
                                    contig_rec_off, dropped, rec_strand, rec_cig_off, cigar, tot, out, batch);
    } catch (const std::exception& e) { set_error(std::string(who) + ": " + e.what()); return HS_EINVAL; }
}

}  // namespace

int hs_realign_intervals(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads,
                         const int32_t* iv_read, const int32_t* iv_contig, const uint8_t* iv_strand, const int32_t* iv_qstart, const int32_t* iv_qend,
                         const int32_t* iv_tstart, const int32_t* iv_tend, int32_t n_intervals, int32_t pad, hs_realign_records** out, hs_cv_batch** batch) {
    return realign_job("hs_realign_intervals", h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, iv_read, iv_contig, iv_strand, iv_qstart, iv_qend, iv_tstart, iv_tend,
                       n_intervals, pad, nullptr, nullptr, nullptr, out, batch);
}

// hs_realign_intervals with every interval cut at its anchors
int hs_realign_intervals_anchored(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads,
                                  const int32_t* iv_read, const int32_t* iv_contig, const uint8_t* iv_strand, const int32_t* iv_qstart, const int32_t* iv_qend,
                                  const int32_t* iv_tstart, const int32_t* iv_tend, int32_t n_intervals, int32_t pad, const int64_t* anc_off, const int32_t* anc_q, const int32_t* anc_t,
                                  hs_realign_records** out, hs_cv_batch** batch) {
    if (int rc = require_device()) return rc;
    if (!anc_off) { set_error("hs_realign_intervals_anchored: bad arguments"); return HS_EINVAL; }
    return realign_job("hs_realign_intervals_anchored", h_contig_seq, h_contig_off, n_contigs, h_read_seq, h_read_off, n_reads, iv_read, iv_contig, iv_strand, iv_qstart, iv_qend, iv_tstart,
                       iv_tend, n_intervals, pad, anc_off, anc_q, anc_t, out, batch);
}


// ---- test taps of the cut and the join (include/hairsplitter_hip.h): the job's own launches on given tables, every table checked before any launch ----
int hs_realign_cut_tap(const uint8_t* seq, int64_t seq_len, const int64_t* off, const int64_t* src, const uint8_t* rev, int32_t m, int32_t fill, uint8_t* out, int64_t out_cap) {
    if (int rc = require_device()) return rc;
    if (!seq || !off || !src || !out || seq_len < 1 || m < 1 || out_cap < 0) { set_error("hs_realign_cut_tap: bad arguments"); return HS_EINVAL; }
    try {
        if (off[0] != 0) { set_error("hs_realign_cut_tap: off must ascend strictly from 0 (off[0] is " + std::to_string(off[0]) + ")"); return HS_EINVAL; }
        for (int32_t i = 0; i < m; ++i) {
            if (off[i + 1] <= off[i] || off[i + 1] > ((int64_t)1 << 40)) { set_error("hs_realign_cut_tap: off must ascend strictly from 0 (piece " + std::to_string(i) + ")"); return HS_EINVAL; }
            const int64_t n = off[i + 1] - off[i];
            const bool r = rev && rev[i];
            // (src inside the sequence first: the piece's other end is then src -+ (n - 1) without overflow)
            if (src[i] < 0 || src[i] >= seq_len || (r ? src[i] - (n - 1) < 0 : src[i] + (n - 1) >= seq_len)) {
                set_error("hs_realign_cut_tap: piece " + std::to_string(i) + " (src " + std::to_string(src[i]) + ", " + std::to_string(n) + " bases, " + (r ? "reversed" : "forward")
                          + ") leaves the sequence [0, " + std::to_string(seq_len) + ")");
                return HS_EINVAL;
            }
        }
        const int64_t total = off[m], out_bytes = (total + 15) & ~(int64_t)15;
        if (out_cap < out_bytes) { set_error("hs_realign_cut_tap: out_cap " + std::to_string(out_cap) + " is below off[m] rounded up to 16 (" + std::to_string(out_bytes) + ")"); return HS_EINVAL; }
        const hipStream_t stream = nullptr;
        DBuf d_seq, d_off, d_src, d_rev, d_out;
        if (int rc = upload_pageable(d_seq, seq, (size_t)seq_len, HS_SEQ_PAD, HS_SEQ_PAD)) return rc;
        const std::vector<int64_t> v_off(off, off + m + 1), v_src(src, src + m);
        std::vector<uint8_t> v_rev;
        if (rev) v_rev.assign(rev, rev + m);
        UploadPack pk;
        pk.add(v_off, d_off); pk.add(v_src, d_src);
        if (rev) pk.add(v_rev, d_rev);
        if (int rc = pk.commit(stream)) return rc;
        if (int rc = d_out.alloc((size_t)out_cap)) return rc;
        if (out_cap) HS_HIP(hipMemsetAsync(d_out.p, fill & 0xff, (size_t)out_cap, stream));
        if (int rc = realign_cut_launch(d_off, d_src, rev ? d_rev.as<uint8_t>() : nullptr, m, total, d_seq.as<uint8_t>() + HS_SEQ_PAD, d_out.as<uint8_t>(), stream)) return rc;
        return d2h_pinned(out, d_out.p, (size_t)out_cap, stream);
    } catch (const std::exception& e) { set_error(std::string("hs_realign_cut_tap: ") + e.what()); return HS_EINVAL; }
}

int hs_anchor_join_tap(int32_t m, const int32_t* iv_piece, const int32_t* iv_base, const int64_t* join_off, const uint8_t* pc_kind, const int32_t* pc_idx, const int32_t* pc_room,
                       const int64_t* pc_ops, const uint8_t* ops, int64_t ops_bytes, const int32_t* dist, const int32_t* start, const int32_t* end, const int32_t* len, int32_t n_num,
                       int32_t fill, int32_t* pc_at, int32_t* out_len, int32_t* out_dist, int32_t* out_pos, uint8_t* joined, int64_t joined_cap) {
    if (int rc = require_device()) return rc;
    if (m < 1 || !iv_piece || !iv_base || !join_off || !pc_kind || !pc_idx || !pc_room || !pc_ops || !ops || ops_bytes < 0 || !dist || !start || !end || !len || n_num < 0 || !pc_at
        || !out_len || !out_dist || !out_pos || !joined || joined_cap < 0) { set_error("hs_anchor_join_tap: bad arguments"); return HS_EINVAL; }
    try {
        const std::string who = "hs_anchor_join_tap: ";
        if (iv_piece[0] != 0 || join_off[0] != 0) { set_error(who + "iv_piece and join_off must ascend from 0"); return HS_EINVAL; }
        for (int32_t k = 0; k < m; ++k) {
            if (iv_piece[k + 1] <= iv_piece[k]) { set_error(who + "interval " + std::to_string(k) + " has no pieces (iv_piece must ascend strictly)"); return HS_EINVAL; }
            if (join_off[k + 1] < join_off[k] || join_off[k + 1] > ((int64_t)1 << 40)) { set_error(who + "join_off must ascend from 0 (interval " + std::to_string(k) + ")"); return HS_EINVAL; }
        }
        for (int32_t k = 0; k < m; ++k) {
            int64_t rooms = 0;
            for (int32_t p = iv_piece[k]; p < iv_piece[k + 1]; ++p) {
                if (pc_kind[p] > hsdev::ANCHOR_INS) { set_error(who + "piece " + std::to_string(p) + " is of kind " + std::to_string(pc_kind[p]) + " (0 .. 4)"); return HS_EINVAL; }
                if (pc_room[p] < 0) { set_error(who + "piece " + std::to_string(p) + " has a negative room"); return HS_EINVAL; }
                if (pc_kind[p] != hsdev::ANCHOR_INS) {
                    if (pc_idx[p] < 0 || pc_idx[p] >= n_num) { set_error(who + "piece " + std::to_string(p) + " names the numbers at " + std::to_string(pc_idx[p]) + " of " + std::to_string(n_num)); return HS_EINVAL; }
                    if (pc_ops[p] < 0 || pc_ops[p] > ops_bytes - pc_room[p]) {
                        set_error(who + "piece " + std::to_string(p) + " has its moves at " + std::to_string(pc_ops[p]) + " + " + std::to_string(pc_room[p]) + " of " + std::to_string(ops_bytes) + " bytes");
                        return HS_EINVAL;
                    }
                }
                rooms += pc_room[p];
            }
            const int64_t room = join_off[k + 1] - join_off[k];
            if (room < rooms || room > 0x7fffffff) {
                set_error(who + "interval " + std::to_string(k) + " has room for " + std::to_string(room) + " moves, its pieces for " + std::to_string(rooms) + " (at least their sum, at most 2^31 - 1)");
                return HS_EINVAL;
            }
        }
        const int64_t joined_bytes = (join_off[m] + 15) & ~(int64_t)15;
        if (joined_cap < joined_bytes) { set_error(who + "joined_cap " + std::to_string(joined_cap) + " is below join_off[m] rounded up to 16 (" + std::to_string(joined_bytes) + ")"); return HS_EINVAL; }
        const size_t P = (size_t)iv_piece[m], M = (size_t)m;
        const hipStream_t stream = nullptr;
        const std::vector<int32_t> v_iv_piece(iv_piece, iv_piece + M + 1), v_iv_base(iv_base, iv_base + M), v_pc_idx(pc_idx, pc_idx + P), v_pc_room(pc_room, pc_room + P);
        const std::vector<int32_t> v_dist(dist, dist + n_num), v_start(start, start + n_num), v_end(end, end + n_num), v_len(len, len + n_num);
        const std::vector<int64_t> v_join_off(join_off, join_off + M + 1), v_pc_ops(pc_ops, pc_ops + P);
        const std::vector<uint8_t> v_pc_kind(pc_kind, pc_kind + P);
        DBuf d_iv_piece, d_iv_base, d_join_off, d_pc_kind, d_pc_idx, d_pc_room, d_pc_ops, d_ops, dd, ds, de, dlen, d_pc_at, d_len, d_dist, d_pos, d_joined;
        UploadPack pk;
        pk.add(v_iv_piece, d_iv_piece); pk.add(v_iv_base, d_iv_base); pk.add(v_join_off, d_join_off); pk.add(v_pc_kind, d_pc_kind); pk.add(v_pc_idx, d_pc_idx); pk.add(v_pc_room, d_pc_room);
        pk.add(v_pc_ops, d_pc_ops); pk.add(v_dist, dd); pk.add(v_start, ds); pk.add(v_end, de); pk.add(v_len, dlen);
        if (int rc = pk.commit(stream)) return rc;
        if (int rc = upload_pageable(d_ops, ops, (size_t)ops_bytes, 0, 16)) return rc;      // (as the job's moves: 16 bytes of room behind them)
        if (int rc = d_pc_at.alloc(P * sizeof(int32_t))) return rc;
        for (DBuf* b : {&d_len, &d_dist, &d_pos}) if (int rc = b->alloc(M * sizeof(int32_t))) return rc;
        if (int rc = d_joined.alloc((size_t)joined_cap)) return rc;
        if (joined_cap) HS_HIP(hipMemsetAsync(d_joined.p, fill & 0xff, (size_t)joined_cap, stream));
        hsdev::AnchorJoinArgs J{};
        J.m = m; J.iv_piece = d_iv_piece.as<int32_t>(); J.iv_base = d_iv_base.as<int32_t>(); J.join_off = d_join_off.as<int64_t>();
        J.pc_kind = d_pc_kind.as<uint8_t>(); J.pc_idx = d_pc_idx.as<int32_t>(); J.pc_room = d_pc_room.as<int32_t>(); J.pc_ops = d_pc_ops.as<int64_t>();
        J.ops = d_ops.as<uint8_t>(); J.dist = dd.as<int32_t>(); J.start = ds.as<int32_t>(); J.end = de.as<int32_t>(); J.len = dlen.as<int32_t>();
        J.pc_at = d_pc_at.as<int32_t>(); J.out_len = d_len.as<int32_t>(); J.out_dist = d_dist.as<int32_t>(); J.out_pos = d_pos.as<int32_t>();
        J.joined = d_joined.as<uint8_t>(); J.joined_bytes = joined_bytes;
        if (int rc = anchor_join_launch(J, stream)) return rc;
        if (int rc = d2h_pinned(pc_at, d_pc_at.p, P * sizeof(int32_t), stream)) return rc;
        if (int rc = d2h_pinned(out_len, d_len.p, M * sizeof(int32_t), stream)) return rc;
        if (int rc = d2h_pinned(out_dist, d_dist.p, M * sizeof(int32_t), stream)) return rc;
        if (int rc = d2h_pinned(out_pos, d_pos.p, M * sizeof(int32_t), stream)) return rc;
        return d2h_pinned(joined, d_joined.p, (size_t)joined_cap, stream);
    } catch (const std::exception& e) { set_error(std::string("hs_anchor_join_tap: ") + e.what()); return HS_EINVAL; }
}

int hs_cv_batch_create_paf(const char* gfa, const char* reads, const char* paf, int32_t n_threads, hs_cv_batch** batch, hs_realign_records** recs) {
    if (int rc = require_device()) return rc;
    if (!gfa || !reads || !paf || !batch) { set_error("hs_cv_batch_create_paf: null argument"); return HS_EINVAL; }
    try {
        if (n_threads < 1) n_threads = host_threads();
        hs::SeqSet seqs;
        if (int rc = hs::load_sequences(gfa, reads, seqs, n_threads)) return rc;
        std::vector<hs::PafRecord> lines;
        long n_unknown = 0;
        if (int rc = hs::parse_paf(paf, seqs, lines, &n_unknown)) return rc;
        if (n_unknown) std::fprintf(stderr, "hairsplitter: realign: %ld PAF lines name a read or a contig that is in neither input file and were left out\n", n_unknown);
        if (lines.size() > 0x7fffffffu || seqs.read_names.size() > 0x7fffffffu) { set_error("hs_cv_batch_create_paf: more than 2^31 PAF lines or reads"); return HS_EINVAL; }
        const size_t n = lines.size();
        std::vector<int32_t> iv_read(n), iv_contig(n), qs(n), qe(n), ts(n), te(n);
        std::vector<uint8_t> strand(n);
        for (size_t i = 0; i < n; ++i) {
            const hs::PafRecord& l = lines[i];
            iv_read[i] = (int32_t)l.read; iv_contig[i] = (int32_t)l.contig; strand[i] = l.minus ? 0 : 1; qs[i] = l.qs; qe[i] = l.qe; ts[i] = l.ts; te[i] = l.te;
        }
        hs_realign_records* r = nullptr;
        if (int rc = hs_realign_intervals(seqs.contig_seq.data(), seqs.contig_off.data(), (int32_t)seqs.contig_names.size(), seqs.read_seq.data(), seqs.read_off.data(),
                                          (int32_t)seqs.read_names.size(), iv_read.data(), iv_contig.data(), strand.data(), qs.data(), qe.data(), ts.data(), te.data(), (int32_t)n,
                                          hs::realign_pad(), &r, batch)) return rc;
        if (recs) *recs = r; else hs_realign_records_destroy(r);
        return HS_OK;
    } catch (const std::exception& e) { set_error(std::string("hs_cv_batch_create_paf: ") + e.what()); return HS_EINVAL; }
}

int hs_cv_batch_create_sam(const char* gfa, const char* reads, const char* sam, int32_t n_threads, hs_cv_batch** batch) {
    if (int rc = require_device()) return rc;
    if (!gfa || !reads || !sam || !batch) { set_error("hs_cv_batch_create_sam: null argument"); return HS_EINVAL; }
    try {
        hs::CvFileInput in;
        if (int rc = hs::load_cv_inputs(gfa, reads, sam, false, in, n_threads < 1 ? host_threads() : n_threads)) return rc;
        return hs_cv_batch_create(in.contig_seq.data(), in.contig_off.data(), (int32_t)in.contig_names.size(), in.read_seq.data(), in.read_off.data(), (int32_t)in.read_names.size(),
                                  in.rec_read.data(), in.rec_pos.data(), in.rec_strand.data(), in.rec_cig_off.data(), in.cigar.data(), in.contig_rec_off.data(), batch);
    } catch (const std::exception& e) { set_error(std::string("hs_cv_batch_create_sam: ") + e.what()); return HS_EINVAL; }
}
