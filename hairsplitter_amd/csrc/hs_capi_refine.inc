// hs_capi_refine.inc -- part of hs_capi.hip: polishing passes (include/hairsplitter_hip.h: hs_polish_haplotypes_refined), the host side of
// hs_kernels_refine.hip. The rule is hs_refine_host.h's. Passes run inside a consensus sub-round of the resident route (consensus_resident) as one
// loop over p: pass 1 votes on the sub-round as it came; when pass p - 1 ends, its text, out_off, ins_len and pieces are on the device (ConsKeep), and pass p is
//   k_refine_windows + two scans -> one shipment of ws, we per piece (16 B; the wait that sizes the buffers: A1's launcher takes host offsets)
//   k_refine_gather twice (queries, targets) -> A1 (hs_edlib_align: NW, PATH, k = -1) in chunks of HS_REALIGN_CHUNK_MB, a wait each
//   moves -> words (MovesToCigar: k_m2c_count, the scan, k_m2c_write; two waits) -> the plan step (cons_plan_step) with k_refine_pieces in front of
//   k_cons_plan, k_cons_layout behind the scans and the pass's sums in the shipment (its wait) -> consensus_round_body on the kept text
//   as backbone (two waits).
// 6 + the A1 chunks waits a pass and sub-round. The intermediate texts never come down.
#include "hs_refine_host.h"

namespace {

// the per-bundle figures of nb bundles into the sums of pass index k
static void refine_add_sums(RefineStats& rs, int k, int64_t nb, const int32_t* n_sub, const int32_t* n_del, const int32_t* n_ins_bases, const int32_t* n_low, const int32_t* n_skipped) {
    for (int64_t b = 0; b < nb; ++b) {
        rs.n_sub[k] += n_sub[b]; rs.n_del[k] += n_del[b]; rs.n_ins_bases[k] += n_ins_bases[b]; rs.n_low[k] += n_low[b]; rs.n_skipped[k] += n_skipped[b];
    }
}

static bool refine_passes_valid(const char* who, int32_t n_passes) {
    if (n_passes >= 1 && n_passes <= HS_REFINE_MAX_PASSES) return true;
    set_error(std::string(who) + ": n_passes is " + std::to_string(n_passes) + ", allowed 1.." + std::to_string(HS_REFINE_MAX_PASSES) + " (HS_REFINE_MAX_PASSES)");
    return false;
}

int refine_sub_round(const char* who, const ConsRound& first, const RefineSubRound& sr, const hs_consensus_params& prm, hipStream_t st, KernelClock& kc, int32_t n_passes,
                     hs::ConsensusHost& H, ConsResidentStats& stats, RefineStats& rs) {
    using namespace hsdev;
    const int64_t nq = first.np, nbs = first.nb;
    auto waits = [] { return (int64_t)g_waits.load(); };
    auto wall = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    ConsKeep keep;             // pass p - 1's text and column arrays
    hs::ConsensusHost Hp;      // its offsets and figures (no text)
    const ConsPiece* d_src = sr.d_src;
    const ConsPiece* d_laid = first.pieces;
    int64_t shift = sr.bundle_shift;
    DBuf d_src_own, d_laid_own;      // pass p - 1's pieces from pass 2 on
    for (int32_t p = 1; p <= n_passes; ++p) {
        const bool last = p == n_passes;
        const int k = p - 1;
        const int64_t w0 = waits();
        // ---- what pass p votes on: the sub-round as it came, or (from pass 2 on) its pieces realigned to pass p - 1's text. A pass realigns the bundles
        // of its sub-round as one round, whatever HS_CONSENSUS_CHUNK_MB: its rows are the windows', a few bytes beside pass 1's
        ConsRound round = first;
        const int32_t* skipped = sr.n_skipped;
        DBuf d_words, d_next, d_laid_next, d_bun, d_tiles;      // (what the round of a later pass points into)
        UploadPack bpk;
        ConsPlanStep plan;
        if (p > 1) {
            const int64_t text_len = Hp.cons_off[(size_t)nbs];
            // ---- the windows, the pairs' lengths and their offsets; 16 bytes a piece come down
            struct { int64_t win, q_len, t_len, q_src, t_src, q_off, t_off, tile_sum, total; } w;
            WorkParts wp;
            w.win = wp.take(nq * (int64_t)sizeof(RefineWin) + 16); w.q_len = wp.take(nq * 4 + 16); w.t_len = wp.take(nq * 4 + 16); w.q_src = wp.take(nq * 8 + 16); w.t_src = wp.take(nq * 8 + 16);
            w.q_off = wp.take((nq + 1) * 8 + 16); w.t_off = wp.take((nq + 1) * 8 + 16); w.tile_sum = wp.take((int64_t)std::max(scan_tiles(nq), 1) * 16);
            w.total = wp.o;
            DBuf d_work;
            if (int rc = d_work.alloc((size_t)w.total)) return rc;
            char* work = (char*)d_work.p;
            RefineWin* d_win = (RefineWin*)(work + w.win);
            int64_t* d_q_off = (int64_t*)(work + w.q_off); int64_t* d_t_off = (int64_t*)(work + w.t_off);
            EventPair ev_win, ev_gather;
            if (int rc = ev_win.take()) return rc;
            if (int rc = ev_gather.take()) return rc;
            if (int rc = timed_launch(kc, ev_win, st, nq * (int64_t)(2 * sizeof(ConsPiece) + sizeof(RefineWin) + 64), [&]() -> int {
                    if (nq) hipLaunchKernelGGL(k_refine_windows, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_src, d_laid, (int)nq, keep.col, keep.slot_index, (long long)keep.n_slots,
                                               keep.ins_len, keep.out_off, d_win, (int32_t*)(work + w.q_len), (int32_t*)(work + w.t_len), (int64_t*)(work + w.q_src), (int64_t*)(work + w.t_src));
                    HS_HIP(hipGetLastError());
                    if (int rc = exclusive_scan_launch((const int32_t*)(work + w.q_len), (int)nq, d_q_off, (long long*)(work + w.tile_sum), st)) return rc;
                    return exclusive_scan_launch((const int32_t*)(work + w.t_len), (int)nq, d_t_off, (long long*)(work + w.tile_sum), st); })) return rc;      // (it takes the tile scratch over: the stream orders it)
            HBuf h_win;
            if (int rc = h_win.alloc((size_t)nq * sizeof(RefineWin) + 16)) return rc;
            Shipment sh;
            sh.add(h_win.p, d_win, (size_t)nq * sizeof(RefineWin));
            if (int rc = sh.launch(st)) return rc;
            if (int rc = stream_wait(st)) return rc;      // the wait for the windows
            stats.moved.down += nq * (int64_t)sizeof(RefineWin);
            // ---- the pairs that go to the aligner, in piece order: their host offsets
            const RefineWin* hw = (const RefineWin*)h_win.p;
            std::vector<int32_t> pair_of((size_t)nq, -1);
            std::vector<int64_t> q_off(1, 0), t_off(1, 0), o_off(1, 0);
            for (int64_t i = 0; i < nq; ++i) {
                const int64_t ws = hw[i].ws, we = hw[i].we, n_bases = sr.h_src[i].n_cols;
                if (!((ws == -1 && we == -1) || (ws >= 0 && ws <= we && we <= text_len))) { set_error(std::string(who) + ": the device's windows do not fit the consensus"); return HS_EHIP; }
                if (ws < 0 || we == ws || n_bases <= 0) continue;
                pair_of[(size_t)i] = (int32_t)(q_off.size() - 1);
                q_off.push_back(q_off.back() + n_bases); t_off.push_back(t_off.back() + (we - ws)); o_off.push_back(o_off.back() + n_bases + (we - ws));
            }
            const int64_t m = (int64_t)q_off.size() - 1, q_total = q_off.back(), t_total = t_off.back();
            rs.n_pairs[k] += m;
            DBuf d_pair_of, d_q, d_t, d_dist, d_start, d_end, d_len, d_ops, d_word_off;
            UploadPack pk;
            pk.add(pair_of, d_pair_of);
            stats.moved.up += (int64_t)pk.total;
            if (int rc = pk.commit(st)) return rc;
            const int64_t q_bytes = (q_total + 15) & ~(int64_t)15, t_bytes = (t_total + 15) & ~(int64_t)15;
            if (int rc = d_q.alloc((size_t)q_bytes + 16)) return rc;
            if (int rc = d_t.alloc((size_t)t_bytes + 16)) return rc;
            for (DBuf* b : {&d_dist, &d_start, &d_end, &d_len}) if (int rc = b->alloc((size_t)std::max<int64_t>(m, 1) * sizeof(int32_t))) return rc;
            if (int rc = d_ops.alloc((size_t)o_off.back() + 16)) return rc;
            if (int rc = d_word_off.alloc((size_t)(m + 1) * sizeof(int64_t))) return rc;
            // ---- the coded queries and targets, pair behind pair
            if (int rc = timed_launch(kc, ev_gather, st, 2 * (q_total + t_total) + 32 * nq, [&]() -> int {
                    if (q_bytes) hipLaunchKernelGGL(k_refine_gather, dim3((unsigned)((q_bytes + 4095) >> 12)), dim3(256), 0, st, d_q_off, (const int64_t*)(work + w.q_src), (int)nq, sr.d_bases,
                                                    d_q.as<uint8_t>(), q_bytes);
                    if (t_bytes) hipLaunchKernelGGL(k_refine_gather, dim3((unsigned)((t_bytes + 4095) >> 12)), dim3(256), 0, st, d_t_off, (const int64_t*)(work + w.t_src), (int)nq, keep.text,
                                                    d_t.as<uint8_t>(), t_bytes);
                    HS_HIP(hipGetLastError());
                    return HS_OK; })) return rc;
            // ---- A1 (synchronous), in chunks bounded as hs_realign_intervals bounds its rounds
            auto t0 = wall();
            const int64_t chunk_bases = (int64_t)hs::realign_chunk_bases();
            for (int64_t k0 = 0; k0 < m;) {
                int64_t k1 = k0 + 1;
                while (k1 < m && o_off[(size_t)k1] - o_off[(size_t)k0] < chunk_bases && k1 - k0 < 1000000) ++k1;
                if (int rc = hs_edlib_align(d_q.as<uint8_t>(), q_off.data() + k0, d_t.as<uint8_t>(), t_off.data() + k0, (int32_t)(k1 - k0), 0, 2, -1, d_dist.as<int32_t>() + k0,
                                            d_start.as<int32_t>() + k0, d_end.as<int32_t>() + k0, nullptr, d_ops.as<uint8_t>(), o_off.data() + k0, d_len.as<int32_t>() + k0, st))
                    return rc;
                k0 = k1;
            }
            rs.t_align_ms[k] += ms_since(t0);
            // ---- moves -> words: a pair without a path gets none; behind them room for the one word of every empty window
            t0 = wall();
            MovesToCigar mc;
            int64_t n_words = 0;
            if (m > 0) { if (int rc = mc.count(d_ops.as<uint8_t>(), o_off.data(), d_len.as<int32_t>(), nullptr, nullptr, (int32_t)m, d_word_off.as<int64_t>(), nullptr, &n_words, st)) return rc; }
            if (n_words < 0 || n_words > o_off.back()) { set_error(std::string(who) + ": the device's word count does not fit the moves"); return HS_EHIP; }
            if (int rc = d_words.alloc((size_t)(n_words + nq + 4) * sizeof(uint32_t))) return rc;
            if (m > 0) { if (int rc = mc.write(d_words.as<uint32_t>(), st)) return rc; }
            rs.t_cigar_ms[k] += ms_since(t0);
            rs.cigar_words[k] += n_words;
            // ---- pass p's bundles (the host knows pass p - 1's offsets and trims), its pieces and their plan
            std::vector<ConsBundle> bun;
            std::vector<ConsTile> tiles;
            if (int rc = cons_round_tables(who, nbs, 0, [&](int64_t b) {
                    const int64_t L = Hp.cons_off[(size_t)b + 1] - Hp.cons_off[(size_t)b];
                    const ConsBundle& ob = (*sr.bundles)[(size_t)b];
                    return ConsBundle{Hp.cons_off[(size_t)b], ob.piece0, ob.piece1, (int32_t)L, hs::refine_overhang_left(Hp.trim_start[(size_t)b]), hs::refine_overhang_right(L, Hp.trim_end[(size_t)b]), 0};
                }, bun, tiles)) return rc;
            bpk.add(bun, d_bun); bpk.add(tiles, d_tiles);
            stats.moved.up += (int64_t)bpk.total;
            if (int rc = bpk.commit(st)) return rc;
            if (int rc = d_next.alloc((size_t)std::max<int64_t>(nq, 1) * sizeof(ConsPiece))) return rc;
            if (int rc = d_laid_next.alloc((size_t)std::max<int64_t>(nq, 1) * sizeof(ConsPiece))) return rc;
            if (int rc = cons_plan_step(who, d_next.as<ConsPiece>(), nq, d_bun.as<ConsBundle>(), bun, d_words.as<uint32_t>(), n_words * 4 + nq * (int64_t)(4 * sizeof(ConsPiece) + sizeof(ConsPlan) + 64),
                                        (int64_t)sizeof(RefineSums), false,
                                        [&](const ConsPlanStep& s) -> int {
                                            if (nq) hipLaunchKernelGGL(k_refine_pieces, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_src, d_laid, (int)nq, (long long)shift, d_win,
                                                                       d_pair_of.as<int32_t>(), d_word_off.as<int64_t>(), (long long)n_words, d_dist.as<int32_t>(), d_len.as<int32_t>(), keep.cons_off,
                                                                       d_words.as<uint32_t>(), d_next.as<ConsPiece>(), (RefineSums*)s.d_extra);
                                            return HS_OK; },
                                        [&](const ConsPlanStep& s) -> int {
                                            if (nq) hipLaunchKernelGGL(k_cons_layout, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_next.as<ConsPiece>(), 0ll, (int)nq, s.d_cols, s.d_recs,
                                                                       s.col_scan, s.rec_scan, 0ll, 0ll, 0ll, d_laid_next.as<ConsPiece>());
                                            HS_HIP(hipGetLastError());
                                            return HS_OK; },
                                        [&](int64_t) { return "pass " + std::to_string(p); }, st, kc, stats.moved, plan)) return rc;
            { float a = 0, b = 0; if (ev_win.ms(&a) == HS_OK && ev_gather.ms(&b) == HS_OK) rs.t_windows_ms[k] += a + b; }
            rs.t_plan_ms[k] += plan.ms;
            int64_t rb = 0, n_rec = 0;
            for (int64_t b = 0; b < nbs; ++b) { rb += plan.bplan[b].row_bytes; n_rec += plan.bplan[b].n_rec; }
            if (int rc = cons_round_fits(who, 0, n_rec)) return rc;
            const RefineSums* sums = (const RefineSums*)plan.extra;
            rs.n_unaligned[k] += sums->n_unaligned; rs.sum_dist[k] += sums->sum_dist; rs.move_bytes[k] += sums->move_bytes;
            // (pass p - 1's text is the backbone)
            round = ConsRound{sr.d_bases, d_words.as<uint32_t>(), keep.text, d_laid_next.as<ConsPiece>(), d_bun.as<ConsBundle>(), d_tiles.as<ConsTile>(),
                              nq, nbs, (int64_t)tiles.size(), rb, n_rec, text_len, sr.n_base, n_words + nq};
            skipped = plan.bskip;
        }
        // ---- the vote: the last pass's into the caller's result with its text; an earlier one's text and column arrays stay on the device for the next
        hs::ConsensusHost Hn;
        Hn.cons_off.assign(1, 0);
        ConsKeep keep_next;
        hs::ConsensusHost& into = last ? H : Hn;
        const size_t at = into.n_sub.size();
        double tms[4] = {0, 0, 0, 0};
        if (int rc = consensus_round_body(who, round, prm, st, kc, tms, into, &stats.moved, last ? nullptr : &keep_next)) return rc;
        refine_add_sums(rs, k, nbs, into.n_sub.data() + at, into.n_del.data() + at, into.n_ins_bases.data() + at, into.n_low.data() + at, skipped);
        if (last) {
            for (int64_t b = 0; b < nbs; ++b) sr.n_skipped_out[b] = skipped[b];
            for (int j = 0; j < 4; ++j) stats.t_ms[j] += tms[j];
        } else {
            // (the body has waited for the stream: nothing reads pass p - 1's blocks any more)
            keep = std::move(keep_next);
            Hp = std::move(Hn);
            if (p > 1) { d_src_own.take(d_next); d_laid_own.take(d_laid_next); d_src = d_src_own.as<ConsPiece>(); d_laid = d_laid_own.as<ConsPiece>(); shift = 0; }
        }
        rs.t_consensus_ms[k] += tms[0] + tms[1] + tms[2] + tms[3];
        rs.n_waits[k] += waits() - w0;
    }
    return HS_OK;
}

// the sums of the call and the last pass's result as the malloc'd result of the C ABI; `last` is taken over (destroyed where the result cannot be made)
static int refined_result_make(const char* who, const RefineStats& rs, int32_t n_passes, hs_haplotypes_result* last, hs_refined_result** out) {
    hs_refined_result* r = static_cast<hs_refined_result*>(std::calloc(1, sizeof(hs_refined_result)));
    if (!r) { hs_haplotypes_result_destroy(last); set_error(std::string(who) + ": out of host memory"); return HS_EINVAL; }
    *r = rs;
    r->last = last; r->n_passes = n_passes;
    *out = r;
    return HS_OK;
}
// pass 1's sums of a one-pass result, and its waits: everything the call waited for that no later pass did
static void refine_first_pass(RefineStats& rs, const hs_consensus_result* c, int32_t n_passes, int64_t waits_of_call) {
    if (n_passes == 1) {
        refine_add_sums(rs, 0, c->n_bundles, c->n_sub, c->n_del, c->n_ins_bases, c->n_low, c->n_skipped);
        rs.t_consensus_ms[0] = c->t_rows_ms + c->t_columns_ms + c->t_ins_ms + c->t_emit_ms;
    }
    rs.n_waits[0] = waits_of_call;
    for (int k = 1; k < n_passes; ++k) rs.n_waits[0] -= rs.n_waits[k];
}
static hs_haplotypes_result* refine_wrap_consensus(hs_consensus_result* c, const ConsResidentStats& stats) {
    hs_haplotypes_result* h = static_cast<hs_haplotypes_result*>(std::calloc(1, sizeof(hs_haplotypes_result)));
    if (!h) { hs_consensus_result_destroy(c); return nullptr; }
    h->consensus = c; h->n_rounds = 1; h->n_sub_rounds = stats.n_sub_rounds; h->bytes_down = stats.moved.down; h->bytes_up = stats.moved.up; h->t_plan_ms = stats.t_plan_ms;
    return h;
}

}  // namespace

extern "C" {

void hs_refined_result_destroy(hs_refined_result* r) {
    if (!r) return;
    hs_haplotypes_result_destroy(r->last);
    std::free(r);
}

int hs_polish_refine_plan_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                               const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                               const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params* params, hs_refine_plan** out) {
    const char* who = "hs_polish_refine_plan_host";
    if (!out) { set_error(std::string(who) + ": bad arguments"); return HS_EINVAL; }
    *out = nullptr;
    try {
        const hs_consensus_params prm = params ? *params : hs_consensus_default_params();
        ConsInput in;
        if (int rc = cons_input_checked(who, ConsInput{n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar}, prm, in))
            return rc;
        hs::RefinePlanHost P;
        std::string err;
        const char* th = std::getenv("HS_CONSENSUS_HOST_THREADS");
        const int n_threads = th ? std::max(1, std::atoi(th)) : hs::host_threads();
        if (int rc = hs::refine_plan_host(in.n_bundles, in.backbone_off, in.backbone, in.ovl, in.ovr, in.piece_off, in.sam, in.flags, in.base_off, in.bases, in.cig_off, in.cigar, prm, n_threads, P, err)) {
            set_error(std::string(who) + ": " + err);
            return rc;
        }
        hs_refine_plan* r = hs::refine_plan_from_host(P);
        if (!r) { set_error(std::string(who) + ": out of host memory"); return HS_EINVAL; }
        r->consensus->n_rounds = 0;
        *out = r;
        return HS_OK;
    } catch (const std::exception& e) { set_error(std::string(who) + ": " + e.what()); return HS_EINVAL; }
}

int hs_polish_refine_arrays(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                            const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                            const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params* params, int32_t n_passes, hs_refined_result** out) {
    const char* who = "hs_polish_refine_arrays";
    if (int rc = require_device()) return rc;
    if (!out) { set_error(std::string(who) + ": bad arguments"); return HS_EINVAL; }
    *out = nullptr;
    if (!refine_passes_valid(who, n_passes)) return HS_EINVAL;
    const hs_consensus_params prm = params ? *params : hs_consensus_default_params();
    try {
        const int64_t waits0 = (int64_t)g_waits.load();
        const ConsInput in{n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar};
        RefineStats rs{};
        ConsResidentStats stats;
        hs_consensus_result* c = nullptr;
        // (one pass is the planned route's call and reports as it does: its sub-rounds, no bytes and no plan time)
        if (int rc = consensus_arrays_resident(who, in, prm, nullptr, &c, n_passes > 1 ? &stats : nullptr, n_passes > 1 ? &rs : nullptr, n_passes)) return rc;
        stats.n_sub_rounds = c->n_rounds;
        refine_first_pass(rs, c, n_passes, (int64_t)g_waits.load() - waits0);
        hs_haplotypes_result* h = refine_wrap_consensus(c, stats);
        if (!h) { set_error(std::string(who) + ": out of host memory"); return HS_EINVAL; }
        return refined_result_make(who, rs, n_passes, h, out);
    } catch (const std::exception& e) { set_error(std::string(who) + ": " + e.what()); return HS_EINVAL; }
}

int hs_polish_haplotypes_refined(hs_cv_batch* b, int32_t c0, int32_t c1, const int64_t* win_off, const int32_t* win_start, const int32_t* win_end, const int64_t* label_off,
                                 const int32_t* labels, const uint8_t* contig_has_snps, int32_t polish_everything, const hs_consensus_params* params, int32_t n_passes,
                                 hs_refined_result** out) {
    const char* who = "hs_polish_haplotypes_refined";
    if (int rc = require_device()) return rc;
    if (!out) { set_error(std::string(who) + ": bad arguments"); return HS_EINVAL; }
    *out = nullptr;
    if (!refine_passes_valid(who, n_passes)) return HS_EINVAL;
    const int64_t waits0 = (int64_t)g_waits.load();
    RefineStats rs{};
    hs_haplotypes_result* h = nullptr;
    // (one pass: the one-pass call itself; more: its body with the passes)
    if (int rc = n_passes == 1 ? hs_polish_haplotypes(b, c0, c1, win_off, win_start, win_end, label_off, labels, contig_has_snps, polish_everything, params, &h)
                               : haplotypes_labels(who, b, c0, c1, win_off, win_start, win_end, label_off, labels, contig_has_snps, polish_everything, params, &h, &rs, n_passes))
        return rc;
    refine_first_pass(rs, h->consensus, n_passes, (int64_t)g_waits.load() - waits0);
    return refined_result_make(who, rs, n_passes, h, out);
}

int hs_polish_haplotypes_refined_from_files(const char* gfa, const char* reads, const char* sam, const char* gro, int32_t polish_everything, const hs_consensus_params* params,
                                            int32_t n_passes, const char* out_fasta, int32_t n_threads) {
    const char* who = "hs_polish_haplotypes_refined_from_files";
    if (!refine_passes_valid(who, n_passes)) return HS_EINVAL;
    if (n_passes == 1) return hs_polish_haplotypes_from_files(gfa, reads, sam, gro, polish_everything, params, out_fasta, n_threads);
    RefineStats rs{};
    return haplotypes_files(who, gfa, reads, sam, gro, polish_everything, params, out_fasta, n_threads, &rs, n_passes);
}

}  // extern "C"
