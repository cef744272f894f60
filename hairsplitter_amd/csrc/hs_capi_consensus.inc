// hs_capi_consensus.inc -- part of hs_capi.hip: the consensus of every polishing bundle (include/hairsplitter_hip.h: hs_polish_consensus), the host
// side of hs_kernels_consensus.hip. The rule is hs_consensus_host.h's. The arrays are the host's (hs_polish_result): the host checks them and
// plans every piece (hs::cons_piece_plan: skipped?, covered columns, voting insertions -- the rows' and the records' places, so no wait for sizes),
// then rounds of whole bundles within HS_CONSENSUS_CHUNK_MB of row bytes go up and through the kernels. Two host waits a round: the number of
// winning slots (their tables are sized by it), the result. Launches are accounted under HS_K_OTHER.

namespace {

struct ConsInput {
    int64_t n_bundles; const int64_t* backbone_off; const uint8_t* backbone; const int32_t* ovl; const int32_t* ovr; const int64_t* piece_off;
    const int32_t* sam; const int32_t* flags; const int64_t* base_off; const uint8_t* bases; const int64_t* cig_off; const uint32_t* cigar;
};

// the work block of a round before the winning slots are known, and the one behind
struct ConsWork { int64_t rows, recs, col, slot_flag, slot_index, out_len, out_off, tile_sum, cons_off, v, total; };
static ConsWork cons_work(int64_t row_bytes, int64_t n_rec, int64_t C, int64_t nb) {
    ConsWork w;
    WorkParts p;
    w.rows = p.take(row_bytes + 16); w.recs = p.take(n_rec * (int64_t)sizeof(hsdev::ConsRecord)); w.col = p.take(C + 16); w.slot_flag = p.take(C * 4);
    w.slot_index = p.take((C + 1) * 8 + 16); w.out_len = p.take(C * 4); w.out_off = p.take((C + 1) * 8 + 16); w.tile_sum = p.take((int64_t)std::max(scan_tiles(C), 1) * 16);
    w.cons_off = p.take((nb + 1) * 8 + 16); w.v = p.take(6 * nb * 4 + 16);
    w.total = p.o;
    return w;
}
struct ConsWork2 { int64_t tab, ins_len, ins_text, text, total; };
static ConsWork2 cons_work2(int64_t W, int32_t max_ins, int64_t text_cap) {
    ConsWork2 w;
    WorkParts p;
    w.tab = p.take(W * hs::cons_table_words(max_ins) * 4); w.ins_len = p.take(W * 4); w.ins_text = p.take(W * max_ins); w.text = p.take(text_cap + 16);
    w.total = p.o;
    return w;
}

int consensus_device(const char* who, const ConsInput& given, const hs_consensus_params& prm, hs_consensus_result** out) {
    using namespace hsdev;
    std::string err;
    ConsInput in = given;
    static const int64_t no_offsets[1] = {0};
    if (in.n_bundles >= 0 && in.piece_off && in.piece_off[in.n_bundles] == 0) { in.base_off = no_offsets; in.cig_off = no_offsets; }      // (a call without pieces may leave them out)
    if (int rc = hs::consensus_check(in.n_bundles, in.backbone_off, in.backbone, in.ovl, in.ovr, in.piece_off, in.sam, in.flags, in.base_off, in.bases, in.cig_off, in.cigar, prm, err)) {
        set_error(std::string(who) + ": " + err);
        return rc;
    }
    const int64_t nb_all = in.n_bundles, n_pieces = in.piece_off[nb_all];
    // ---- the plan of every piece, on the host's threads
    std::vector<hs::ConsPiecePlan> plan((size_t)n_pieces);
    std::vector<int32_t> piece_bundle((size_t)n_pieces);
    for (int64_t b = 0; b < nb_all; ++b) for (int64_t p = in.piece_off[b]; p < in.piece_off[b + 1]; ++p) piece_bundle[(size_t)p] = (int32_t)b;
    const int parts = (int)std::min<int64_t>(std::max<int64_t>(n_pieces / 256, 1), 4096);
    hs::hs_parallel_for(parts, std::min(parts, host_threads()), [&](int q) {
        for (int64_t p = n_pieces * q / parts; p < n_pieces * (q + 1) / parts; ++p) {
            const int64_t b = piece_bundle[(size_t)p];
            plan[(size_t)p] = hs::cons_piece_plan(in.cigar + in.cig_off[p], in.cig_off[p + 1] - in.cig_off[p], in.base_off[p + 1] - in.base_off[p], in.flags[p], in.sam[p],
                                                  in.backbone_off[b + 1] - in.backbone_off[b]);
        }
    });
    std::vector<int64_t> row_bytes((size_t)nb_all, 0);
    hs::ConsensusHost H;      // the result as it grows, round by round
    H.cons_off.assign(1, 0);
    H.n_skipped.assign((size_t)nb_all, 0);
    for (int64_t p = 0; p < n_pieces; ++p) {
        const int64_t b = piece_bundle[(size_t)p];
        if (plan[(size_t)p].long_cigar) { set_error(std::string(who) + ": bundle " + std::to_string(b) + ": a CIGAR of more than 2^31 - 1 bases"); return HS_EINVAL; }
        if (plan[(size_t)p].skipped) H.n_skipped[(size_t)b]++;
        row_bytes[(size_t)b] += plan[(size_t)p].n_cols;
    }
    const char* bud = std::getenv("HS_CONSENSUS_CHUNK_MB");
    const int64_t budget = std::max<int64_t>(1, bud ? std::atoll(bud) : 1024) * (1 << 20), max_cols = (int64_t)1 << 30;
    for (int64_t b = 0; b < nb_all; ++b)
        if (row_bytes[(size_t)b] > budget) {
            set_error(std::string(who) + ": bundle " + std::to_string(b) + " alone takes " + std::to_string(row_bytes[(size_t)b]) + " row bytes, more than HS_CONSENSUS_CHUNK_MB allows");
            return HS_EINVAL;
        }

    hipStream_t st = nullptr;
    KernelClock kc;
    double t_ms[4] = {0, 0, 0, 0};
    int64_t n_rounds = 0;
    for (int64_t b0 = 0; b0 < nb_all;) {
        int64_t b1 = b0, rb = 0, C = 0;
        while (b1 < nb_all) {      // whole bundles; at least one
            const int64_t L = in.backbone_off[b1 + 1] - in.backbone_off[b1];
            if (b1 > b0 && (rb + row_bytes[(size_t)b1] > budget || C + L > max_cols)) break;
            rb += row_bytes[(size_t)b1]; C += L; ++b1;
        }
        ++n_rounds;
        const int64_t nb = b1 - b0, p0 = in.piece_off[b0], p1 = in.piece_off[b1], np = p1 - p0;
        const int64_t base0 = in.base_off[p0], cig0 = in.cig_off[p0], bb0 = in.backbone_off[b0];
        // ---- the round's tables
        std::vector<ConsPiece> pieces((size_t)np);
        std::vector<ConsBundle> bundles((size_t)nb);
        std::vector<ConsTile> tiles;
        int64_t n_rec = 0, row_at = 0;
        for (int64_t b = b0; b < b1; ++b) {
            const int64_t L = in.backbone_off[b + 1] - in.backbone_off[b], col_off = in.backbone_off[b] - bb0;
            bundles[(size_t)(b - b0)] = ConsBundle{col_off, (int32_t)(in.piece_off[b] - p0), (int32_t)(in.piece_off[b + 1] - p0), (int32_t)L, in.ovl[b], in.ovr[b], 0};
            for (int64_t t0 = 0; t0 < L; t0 += 256) tiles.push_back(ConsTile{(int32_t)(b - b0), (int32_t)t0});
            for (int64_t p = in.piece_off[b]; p < in.piece_off[b + 1]; ++p) {
                const hs::ConsPiecePlan& pl = plan[(size_t)p];
                pieces[(size_t)(p - p0)] = ConsPiece{in.base_off[p] - base0, in.cig_off[p] - cig0, row_at, n_rec, col_off, (int32_t)(in.cig_off[p + 1] - in.cig_off[p]), in.sam[p] - 1,
                                                     pl.skipped ? 0 : pl.n_cols, pl.skipped ? 0 : pl.n_ins};
                if (!pl.skipped) { row_at += pl.n_cols; n_rec += pl.n_ins; }
            }
        }
        if (tiles.size() > (size_t)0x7fffffff || n_rec > 0x7fffffff - 256) { set_error(std::string(who) + ": a round is too large; lower HS_CONSENSUS_CHUNK_MB"); return HS_EINVAL; }
        DBuf d_pieces, d_bundles, d_tiles, d_bases, d_cigar, d_bb, d_work, d_work2;
        UploadPack pk;
        pk.add(pieces, d_pieces); pk.add(bundles, d_bundles); pk.add(tiles, d_tiles);
        if (int rc = pk.commit(st)) return rc;
        if (int rc = upload_pageable(d_bases, in.bases ? in.bases + base0 : nullptr, (size_t)(in.base_off[p1] - base0), 0, 16)) return rc;
        if (int rc = upload_pageable(d_cigar, in.cigar ? in.cigar + cig0 : nullptr, (size_t)(in.cig_off[p1] - cig0) * 4, 0, 16)) return rc;
        if (int rc = upload_pageable(d_bb, in.backbone ? in.backbone + bb0 : nullptr, (size_t)C, 0, 16)) return rc;
        const ConsWork w = cons_work(rb, n_rec, C, nb);
        if (int rc = d_work.alloc((size_t)w.total)) return rc;
        char* work = (char*)d_work.p;
        uint8_t* rows = (uint8_t*)(work + w.rows); ConsRecord* recs = (ConsRecord*)(work + w.recs); uint8_t* col = (uint8_t*)(work + w.col);
        int32_t* slot_flag = (int32_t*)(work + w.slot_flag); int64_t* slot_index = (int64_t*)(work + w.slot_index); int32_t* out_len = (int32_t*)(work + w.out_len);
        int64_t* out_off = (int64_t*)(work + w.out_off); long long* tile_sum = (long long*)(work + w.tile_sum);
        int64_t* d_cons_off = (int64_t*)(work + w.cons_off); int32_t* d_v = (int32_t*)(work + w.v);
        EventPair ev[4];
        for (EventPair& e : ev) if (int rc = e.init()) return rc;

        // ---- rows and records; columns; the winning slots numbered -- and counted (the first wait)
        if (int rc = timed_launch(kc, ev[0], st, (in.cig_off[p1] - cig0) * 4 + (in.base_off[p1] - base0) + rb + n_rec * (int64_t)sizeof(ConsRecord), [&]() -> int {
                if (n_rec) HS_HIP(hipMemsetAsync(recs, 0xFF, (size_t)n_rec * sizeof(ConsRecord), st));      // (a record the plan counted and the walk did not write: slot -1)
                if (np) hipLaunchKernelGGL(k_cons_rows, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, st, d_pieces.as<ConsPiece>(), (int)np, d_cigar.as<uint32_t>(), d_bases.as<uint8_t>(),
                                           prm.max_ins, rows, recs);
                HS_HIP(hipGetLastError());
                return HS_OK; })) return rc;
        if (int rc = timed_launch(kc, ev[1], st, rb + 6 * C + 32 * np, [&]() -> int {
                if (!tiles.empty()) hipLaunchKernelGGL(k_cons_columns, dim3((unsigned)tiles.size()), dim3(256), 0, st, d_tiles.as<ConsTile>(), d_bundles.as<ConsBundle>(),
                                                       d_pieces.as<ConsPiece>(), rows, d_bb.as<uint8_t>(), prm.min_cov, col, slot_flag);
                HS_HIP(hipGetLastError());
                return exclusive_scan_launch(slot_flag, (int)C, slot_index, tile_sum, st); })) return rc;
        HBuf h_word;
        if (int rc = h_word.alloc(32)) return rc;
        Shipment sh1;
        const int64_t* h_W = sh1.add_word(h_word.p, slot_index + C);
        if (int rc = sh1.launch(st, 1)) return rc;
        if (int rc = stream_wait(st)) return rc;
        const int64_t W = *h_W;
        if (W < 0 || W > C || W > n_rec) { set_error(std::string(who) + ": the device's slot count does not fit the records"); return HS_EHIP; }

        // ---- the tables of the winning slots, their decisions; lengths, scan, text, the bundles' figures; one shipment (the second wait)
        const int64_t text_cap = C + W * prm.max_ins;
        const ConsWork2 w2 = cons_work2(W, prm.max_ins, text_cap);
        if (int rc = d_work2.alloc((size_t)w2.total)) return rc;
        char* work2 = (char*)d_work2.p;
        uint32_t* tab = (uint32_t*)(work2 + w2.tab); int32_t* ins_len = (int32_t*)(work2 + w2.ins_len); uint8_t* ins_text = (uint8_t*)(work2 + w2.ins_text);
        uint8_t* text = (uint8_t*)(work2 + w2.text);
        if (int rc = timed_launch(kc, ev[2], st, n_rec * (int64_t)sizeof(ConsRecord) + W * hs::cons_table_words(prm.max_ins) * 8 + 5 * C, [&]() -> int {
                if (W) HS_HIP(hipMemsetAsync(work2 + w2.tab, 0, (size_t)(w2.ins_text - w2.tab), st));      // (tables and lengths)
                if (W && n_rec) hipLaunchKernelGGL(k_cons_ins_vote, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, recs, (long long)n_rec, col, slot_index, (long long)W,
                                                   d_bases.as<uint8_t>(), prm.max_ins, tab);
                if (C) hipLaunchKernelGGL(k_cons_ins_decide, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, col, (long long)C, slot_index, (long long)W, tab, prm.max_ins, ins_len,
                                          ins_text, out_len);
                HS_HIP(hipGetLastError());
                return HS_OK; })) return rc;
        if (int rc = timed_launch(kc, ev[3], st, 22 * C + 2 * text_cap, [&]() -> int {
                if (int rc = exclusive_scan_launch(out_len, (int)C, out_off, tile_sum, st)) return rc;
                if (C) hipLaunchKernelGGL(k_cons_emit, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, col, (long long)C, d_bb.as<uint8_t>(), slot_index, (long long)W, ins_len, ins_text,
                                          prm.max_ins, out_off, (long long)text_cap, text);
                hipLaunchKernelGGL(k_cons_bundles, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, d_bundles.as<ConsBundle>(), (int)nb, col, slot_index, (long long)W, ins_len, out_off,
                                   d_cons_off, d_v);
                HS_HIP(hipGetLastError());
                return HS_OK; })) return rc;
        HBuf h_text, h_off, h_v;
        if (int rc = h_text.alloc((size_t)text_cap + 16)) return rc;
        if (int rc = h_off.alloc((size_t)(nb + 1) * 8 + 16)) return rc;
        if (int rc = h_v.alloc((size_t)(6 * nb) * 4 + 16)) return rc;
        Shipment sh2;
        if (text_cap > 0) sh2.add_counted(h_text.p, text, (const long long*)(out_off + C), 1, (long long)text_cap);
        sh2.add(h_off.p, d_cons_off, (size_t)(nb + 1) * 8);
        sh2.add(h_v.p, d_v, (size_t)(6 * nb) * 4);
        if (int rc = sh2.launch(st)) return rc;
        if (int rc = stream_wait(st)) return rc;
        kc.flush();
        for (int k = 0; k < 4; ++k) { float ms = 0; if (ev[k].ms(&ms) == HS_OK) t_ms[k] += ms; }

        // ---- the round into the result
        const int64_t* co = (const int64_t*)h_off.p;
        bool ok = co[0] == 0 && co[nb] >= 0 && co[nb] <= text_cap;
        for (int64_t k = 0; ok && k < nb; ++k) ok = co[k + 1] >= co[k];
        if (!ok) { set_error(std::string(who) + ": the device's consensus offsets do not fit the columns"); return HS_EHIP; }
        const int64_t at = (int64_t)H.cons.size();
        H.cons.insert(H.cons.end(), (const uint8_t*)h_text.p, (const uint8_t*)h_text.p + co[nb]);
        for (int64_t k = 0; k < nb; ++k) H.cons_off.push_back(at + co[k + 1]);
        const int32_t* v = (const int32_t*)h_v.p;
        std::vector<int32_t>* f[6] = {&H.trim_start, &H.trim_end, &H.n_sub, &H.n_del, &H.n_ins_bases, &H.n_low};
        for (int j = 0; j < 6; ++j) f[j]->insert(f[j]->end(), v + j * nb, v + (j + 1) * nb);
        H.n_ins_records += n_rec; H.n_ins_slots += W;
        b0 = b1;
    }
    hs_consensus_result* r = hs::consensus_result_from_host(H);
    if (!r) { set_error(std::string(who) + ": out of host memory"); return HS_EINVAL; }
    r->t_rows_ms = t_ms[0]; r->t_columns_ms = t_ms[1]; r->t_ins_ms = t_ms[2]; r->t_emit_ms = t_ms[3]; r->n_rounds = n_rounds;
    *out = r;
    return HS_OK;
}

}  // namespace

extern "C" {

int hs_polish_consensus_arrays(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                               const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                               const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params* params, hs_consensus_result** out) {
    if (int rc = require_device()) return rc;
    if (!out) { set_error("hs_polish_consensus: bad arguments"); return HS_EINVAL; }
    *out = nullptr;
    const ConsInput in{n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar};
    try { return consensus_device("hs_polish_consensus", in, params ? *params : hs_consensus_default_params(), out); }
    catch (const std::exception& e) { set_error(std::string("hs_polish_consensus: ") + e.what()); return HS_EINVAL; }
}

int hs_polish_consensus(const hs_polish_result* in, const hs_consensus_params* params, hs_consensus_result** out) {
    if (!in) { set_error("hs_polish_consensus: bad arguments"); return HS_EINVAL; }
    return hs_polish_consensus_arrays(in->n_bundles, in->backbone_off, in->backbone, in->bundle_overhang_left, in->bundle_overhang_right, in->piece_off, in->piece_sam_pos,
                                      in->piece_flags, in->base_off, in->bases, in->cig_off, in->cigar, params, out);
}

int hs_polish_consensus_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                             const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                             const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params* params, hs_consensus_result** out) {
    if (!out) { set_error("hs_polish_consensus_host: bad arguments"); return HS_EINVAL; }
    *out = nullptr;
    try {
        hs::ConsensusHost H;
        std::string err;
        const char* th = std::getenv("HS_CONSENSUS_HOST_THREADS");
        const int n_threads = th ? std::max(1, std::atoi(th)) : hs::host_threads();
        if (int rc = hs::consensus_host(n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar,
                                        params ? *params : hs_consensus_default_params(), n_threads, H, err)) {
            set_error("hs_polish_consensus_host: " + err);
            return rc;
        }
        hs_consensus_result* r = hs::consensus_result_from_host(H);
        if (!r) { set_error("hs_polish_consensus_host: out of host memory"); return HS_EINVAL; }
        r->n_rounds = 0;
        *out = r;
        return HS_OK;
    } catch (const std::exception& e) { set_error(std::string("hs_polish_consensus_host: ") + e.what()); return HS_EINVAL; }
}

}  // extern "C"
