// hs_capi_consensus.inc -- part of hs_capi.hip: the consensus of every polishing bundle (include/hairsplitter_hip.h: hs_polish_consensus), the host
// side of hs_kernels_consensus.hip. The rule is hs_consensus_host.h's. The arrays are the host's (hs_polish_result): the host checks them and
// plans every piece (hs::cons_piece_plan: skipped?, covered columns, voting insertions -- the rows' and the records' places, so no wait for sizes),
// then rounds of whole bundles within HS_CONSENSUS_CHUNK_MB of row bytes go up and through the kernels. Two host waits a round: the number of
// winning slots (their tables are sized by it), the result. Launches are accounted under HS_K_OTHER.
// Behind it the resident route (consensus_resident, hs_polish_haplotypes): the pieces hs_polish_inputs' kernels cut stay on the device, k_cons_plan
// plans them there (cons_plan_step: one wait for the sizes), and both routes end in the same round body.
// What both routes and the polishing passes (hs_capi_refine.inc) share is stated once: the checked input (cons_input_checked), the rounds'
// cut (cons_budget, cons_cut_round), a round's tables (cons_round_tables), the plan step, the result's ending (cons_result_finish).

#include "hs_haplotypes_host.h"

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

// a round on the device: whole bundles whose tables, bases, CIGAR words and backbone text are there, every offset counted from the round's
// own beginning. The arrays' route (consensus_device) uploads them from the host; the resident route (consensus_resident) points into the
// buffers hs_polish_inputs' kernels filled.
struct ConsRound {
    const uint8_t* bases; const uint32_t* cigar; const uint8_t* bb; const hsdev::ConsPiece* pieces; const hsdev::ConsBundle* bundles; const hsdev::ConsTile* tiles;
    int64_t np, nb, n_tiles, rb /* row bytes */, n_rec, C /* columns */, n_base, n_cig;
};

// what a round leaves on the device for a caller that goes on with it (the polishing passes, hs_capi_refine.inc): its two work blocks and, inside
// them, the text, the decided columns, the winning slots and their lengths, the text offset of every column and of every bundle
struct ConsKeepViews {
    const uint8_t* text = nullptr; const uint8_t* col = nullptr; const int64_t* slot_index = nullptr; const int32_t* ins_len = nullptr; const int64_t* out_off = nullptr;
    const int64_t* cons_off = nullptr;
    int64_t n_slots = 0, text_cap = 0;
};
struct ConsKeep : ConsKeepViews {
    DBuf work, work2;
    ConsKeep() = default;
    ConsKeep& operator=(ConsKeep&& o) { ConsKeepViews::operator=(o); work.take(o.work); work2.take(o.work2); return *this; }      // (the blocks change hands)
};

// from k_cons_rows to "the round into the result": two host waits. keep (null: as ever): the text stays on the device and the blocks go to *keep; the
// bundles' offsets and figures come down as ever and H grows by them, not by text
int consensus_round_body(const char* who, const ConsRound& r, const hs_consensus_params& prm, hipStream_t st, KernelClock& kc, double t_ms[4], hs::ConsensusHost& H,
                         BytesMoved* moved = nullptr, ConsKeep* keep = nullptr) {
    using namespace hsdev;
    const int64_t np = r.np, nb = r.nb, rb = r.rb, n_rec = r.n_rec, C = r.C;
    DBuf d_work, d_work2;
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
    if (int rc = timed_launch(kc, ev[0], st, r.n_cig * 4 + r.n_base + rb + n_rec * (int64_t)sizeof(ConsRecord), [&]() -> int {
            if (n_rec) HS_HIP(hipMemsetAsync(recs, 0xFF, (size_t)n_rec * sizeof(ConsRecord), st));      // (a record the plan counted and the walk did not write: slot -1)
            if (np) hipLaunchKernelGGL(k_cons_rows, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, st, r.pieces, (int)np, r.cigar, r.bases, prm.max_ins, rows, recs);
            HS_HIP(hipGetLastError());
            return HS_OK; })) return rc;
    if (int rc = timed_launch(kc, ev[1], st, rb + 6 * C + 32 * np, [&]() -> int {
            if (r.n_tiles) hipLaunchKernelGGL(k_cons_columns, dim3((unsigned)r.n_tiles), dim3(256), 0, st, r.tiles, r.bundles, r.pieces, rows, r.bb, prm.min_cov, col, slot_flag);
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
                                               r.bases, prm.max_ins, tab);
            if (C) hipLaunchKernelGGL(k_cons_ins_decide, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, col, (long long)C, slot_index, (long long)W, tab, prm.max_ins, ins_len,
                                      ins_text, out_len);
            HS_HIP(hipGetLastError());
            return HS_OK; })) return rc;
    if (int rc = timed_launch(kc, ev[3], st, 22 * C + 2 * text_cap, [&]() -> int {
            if (int rc = exclusive_scan_launch(out_len, (int)C, out_off, tile_sum, st)) return rc;
            if (C) hipLaunchKernelGGL(k_cons_emit, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, col, (long long)C, r.bb, slot_index, (long long)W, ins_len, ins_text,
                                      prm.max_ins, out_off, (long long)text_cap, text);
            hipLaunchKernelGGL(k_cons_bundles, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, r.bundles, (int)nb, col, slot_index, (long long)W, ins_len, out_off,
                               d_cons_off, d_v);
            HS_HIP(hipGetLastError());
            return HS_OK; })) return rc;
    HBuf h_text, h_off, h_v;
    if (!keep) { if (int rc = h_text.alloc((size_t)text_cap + 16)) return rc; }
    if (int rc = h_off.alloc((size_t)(nb + 1) * 8 + 16)) return rc;
    if (int rc = h_v.alloc((size_t)(6 * nb) * 4 + 16)) return rc;
    Shipment sh2;
    if (text_cap > 0 && !keep) sh2.add_counted(h_text.p, text, (const long long*)(out_off + C), 1, (long long)text_cap);
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
    if (!keep) H.cons.insert(H.cons.end(), (const uint8_t*)h_text.p, (const uint8_t*)h_text.p + co[nb]);
    for (int64_t k = 0; k < nb; ++k) H.cons_off.push_back(at + co[k + 1]);
    const int32_t* v = (const int32_t*)h_v.p;
    std::vector<int32_t>* f[6] = {&H.trim_start, &H.trim_end, &H.n_sub, &H.n_del, &H.n_ins_bases, &H.n_low};
    for (int j = 0; j < 6; ++j) f[j]->insert(f[j]->end(), v + j * nb, v + (j + 1) * nb);
    H.n_ins_records += n_rec; H.n_ins_slots += W;
    if (moved) moved->down += 16 + (keep ? 0 : co[nb]) + (nb + 1) * 8 + 6 * nb * 4;
    if (keep) {
        static_cast<ConsKeepViews&>(*keep) = ConsKeepViews{text, col, slot_index, ins_len, out_off, d_cons_off, W, text_cap};
        keep->work.take(d_work); keep->work2.take(d_work2);
    }
    return HS_OK;
}

// ---- what the routes share ------------------------------------------------------------------------------------------------------------------
// the arrays of a call as every route reads them: a call without pieces may leave base_off and cig_off out; then hs::consensus_check
static int cons_input_checked(const char* who, const ConsInput& given, const hs_consensus_params& prm, ConsInput& in) {
    in = given;
    if (in.n_bundles >= 0 && in.piece_off && in.piece_off[in.n_bundles] == 0) { static const int64_t no_offsets[1] = {0}; in.base_off = in.cig_off = no_offsets; }
    std::string err;
    const int rc = hs::consensus_check(in.n_bundles, in.backbone_off, in.backbone, in.ovl, in.ovr, in.piece_off, in.sam, in.flags, in.base_off, in.bases, in.cig_off, in.cigar, prm, err);
    if (rc) set_error(std::string(who) + ": " + err);
    return rc;
}

// the row bytes a round may hold
static int64_t cons_budget() {
    const char* bud = std::getenv("HS_CONSENSUS_CHUNK_MB");
    return std::max<int64_t>(1, bud ? std::atoll(bud) : 1024) * (1 << 20);
}
// the next round of z: whole bundles [s0, cut.s1), at least one, within the budget and 2^30 columns, and their sums. The first call (s0 == 0)
// refuses a bundle that no round can hold, before anything runs; it is named by its place in the call, first_named + its place in z
struct ConsBundleSize { int64_t row_bytes, n_rec, L; };
struct ConsCut { int64_t s1, rb, n_rec, C; };
static int cons_cut_round(const char* who, const std::vector<ConsBundleSize>& z, int64_t first_named, int64_t s0, ConsCut& cut) {
    const int64_t budget = cons_budget(), max_cols = (int64_t)1 << 30, n = (int64_t)z.size();
    for (int64_t k = 0; s0 == 0 && k < n; ++k)
        if (z[(size_t)k].row_bytes > budget) {
            set_error(std::string(who) + ": bundle " + std::to_string(first_named + k) + " alone takes " + std::to_string(z[(size_t)k].row_bytes) + " row bytes, more than HS_CONSENSUS_CHUNK_MB allows");
            return HS_EINVAL;
        }
    cut = ConsCut{s0, 0, 0, 0};
    for (; cut.s1 < n; ++cut.s1) {
        const ConsBundleSize& b = z[(size_t)cut.s1];
        if (cut.s1 > s0 && (cut.rb + b.row_bytes > budget || cut.C + b.L > max_cols)) break;
        cut.rb += b.row_bytes; cut.n_rec += b.n_rec; cut.C += b.L;
    }
    return HS_OK;
}

// the one size check of a round: what the kernels index with an int
static int cons_round_fits(const char* who, size_t n_tiles, int64_t n_rec) {
    if (n_tiles <= (size_t)0x7fffffff && n_rec <= 0x7fffffff - 256) return HS_OK;
    set_error(std::string(who) + ": a round is too large; lower HS_CONSENSUS_CHUNK_MB");
    return HS_EINVAL;
}
// the bundles of a round -- bundle_at(k): column offset, piece range, L and overhangs, counted from the round's beginning -- and a tile per 256 columns
template <class BundleAt>
static int cons_round_tables(const char* who, int64_t nb, int64_t n_rec, BundleAt bundle_at, std::vector<hsdev::ConsBundle>& bundles, std::vector<hsdev::ConsTile>& tiles) {
    bundles.resize((size_t)nb);
    for (int64_t k = 0; k < nb; ++k) {
        bundles[(size_t)k] = bundle_at(k);
        for (int64_t t0 = 0; t0 < bundles[(size_t)k].L; t0 += 256) tiles.push_back(hsdev::ConsTile{(int32_t)k, (int32_t)t0});
    }
    return cons_round_fits(who, tiles.size(), n_rec);
}

// a result of the C ABI from H, the four kernel times and the number of rounds (null: out of host memory, named)
static hs_consensus_result* cons_result_finish(const char* who, const hs::ConsensusHost& H, const double t_ms[4], int64_t n_rounds) {
    hs_consensus_result* r = hs::consensus_result_from_host(H);
    if (!r) { set_error(std::string(who) + ": out of host memory"); return nullptr; }
    r->t_rows_ms = t_ms[0]; r->t_columns_ms = t_ms[1]; r->t_ins_ms = t_ms[2]; r->t_emit_ms = t_ms[3]; r->n_rounds = n_rounds;
    return r;
}

int consensus_device(const char* who, const ConsInput& given, const hs_consensus_params& prm, hs_consensus_result** out) {
    using namespace hsdev;
    ConsInput in;
    if (int rc = cons_input_checked(who, given, prm, in)) return rc;
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
    std::vector<ConsBundleSize> sizes((size_t)nb_all);
    for (int64_t b = 0; b < nb_all; ++b) sizes[(size_t)b] = ConsBundleSize{0, 0, in.backbone_off[b + 1] - in.backbone_off[b]};
    hs::ConsensusHost H;      // the result as it grows, round by round
    H.cons_off.assign(1, 0);
    H.n_skipped.assign((size_t)nb_all, 0);
    for (int64_t p = 0; p < n_pieces; ++p) {
        const int64_t b = piece_bundle[(size_t)p];
        const hs::ConsPiecePlan& pl = plan[(size_t)p];
        if (pl.long_cigar) { set_error(std::string(who) + ": bundle " + std::to_string(b) + ": a CIGAR of more than 2^31 - 1 bases"); return HS_EINVAL; }
        if (pl.skipped) H.n_skipped[(size_t)b]++; else sizes[(size_t)b].n_rec += pl.n_ins;
        sizes[(size_t)b].row_bytes += pl.n_cols;
    }

    hipStream_t st = nullptr;
    KernelClock kc;
    double t_ms[4] = {0, 0, 0, 0};
    int64_t n_rounds = 0;
    ConsCut cut;
    for (int64_t b0 = 0; b0 < nb_all; b0 = cut.s1) {
        if (int rc = cons_cut_round(who, sizes, 0, b0, cut)) return rc;
        ++n_rounds;
        const int64_t b1 = cut.s1, nb = b1 - b0, p0 = in.piece_off[b0], p1 = in.piece_off[b1], np = p1 - p0;
        const int64_t base0 = in.base_off[p0], cig0 = in.cig_off[p0], bb0 = in.backbone_off[b0];
        // ---- the round's tables
        std::vector<ConsPiece> pieces((size_t)np);
        std::vector<ConsBundle> bundles;
        std::vector<ConsTile> tiles;
        if (int rc = cons_round_tables(who, nb, cut.n_rec, [&](int64_t k) {
                const int64_t b = b0 + k;
                return ConsBundle{in.backbone_off[b] - bb0, (int32_t)(in.piece_off[b] - p0), (int32_t)(in.piece_off[b + 1] - p0), (int32_t)sizes[(size_t)b].L, in.ovl[b], in.ovr[b], 0};
            }, bundles, tiles)) return rc;
        int64_t rec_at = 0, row_at = 0;
        for (int64_t p = p0; p < p1; ++p) {
            const hs::ConsPiecePlan& pl = plan[(size_t)p];
            pieces[(size_t)(p - p0)] = ConsPiece{in.base_off[p] - base0, in.cig_off[p] - cig0, row_at, rec_at, bundles[(size_t)(piece_bundle[(size_t)p] - b0)].col_off,
                                                 (int32_t)(in.cig_off[p + 1] - in.cig_off[p]), in.sam[p] - 1, pl.skipped ? 0 : pl.n_cols, pl.skipped ? 0 : pl.n_ins};
            if (!pl.skipped) { row_at += pl.n_cols; rec_at += pl.n_ins; }
        }
        DBuf d_pieces, d_bundles, d_tiles, d_bases, d_cigar, d_bb;
        UploadPack pk;
        pk.add(pieces, d_pieces); pk.add(bundles, d_bundles); pk.add(tiles, d_tiles);
        if (int rc = pk.commit(st)) return rc;
        if (int rc = upload_pageable(d_bases, in.bases ? in.bases + base0 : nullptr, (size_t)(in.base_off[p1] - base0), 0, 16)) return rc;
        if (int rc = upload_pageable(d_cigar, in.cigar ? in.cigar + cig0 : nullptr, (size_t)(in.cig_off[p1] - cig0) * 4, 0, 16)) return rc;
        if (int rc = upload_pageable(d_bb, in.backbone ? in.backbone + bb0 : nullptr, (size_t)cut.C, 0, 16)) return rc;
        const ConsRound round{d_bases.as<uint8_t>(), d_cigar.as<uint32_t>(), d_bb.as<uint8_t>(), d_pieces.as<ConsPiece>(), d_bundles.as<ConsBundle>(), d_tiles.as<ConsTile>(),
                              np, nb, (int64_t)tiles.size(), cut.rb, cut.n_rec, cut.C, in.base_off[p1] - base0, in.cig_off[p1] - cig0};
        if (int rc = consensus_round_body(who, round, prm, st, kc, t_ms, H)) return rc;
    }
    *out = cons_result_finish(who, H, t_ms, n_rounds);
    return *out ? HS_OK : HS_EINVAL;
}

// ---- the plan step of the resident route and of every polishing pass: k_cons_plan plans np pieces against their bundles, two scans lay the
// rows and the records out, and one shipment brings the sizes to the host -- one wait. The ship block, stated here alone:
//   first_long (16 bytes) | ConsBundlePlan[nb] | extra_bytes of the caller's (a pass's RefineSums) | n_skipped[nb]
// The step checks what came down against the bundles and refuses a CIGAR of more than 2^31 - 1 bases; named(piece) says whose it is.
// before / after (either may be empty) launch in front of k_cons_plan and behind the scans, inside the step's one timed launch.
struct ConsPlanStep {
    DBuf work; HBuf ship, plan;      // the owners; plan: ConsPlan[np] on the host, where asked for
    const hsdev::ConsBundlePlan* bplan = nullptr; const char* extra = nullptr; const int32_t* bskip = nullptr;      // host views of the ship block
    int32_t* d_cols = nullptr; int32_t* d_recs = nullptr; int64_t* col_scan = nullptr; int64_t* rec_scan = nullptr; char* d_extra = nullptr;
    float ms = 0;
};
using ConsPlanHook = std::function<int(const ConsPlanStep&)>;
int cons_plan_step(const char* who, const hsdev::ConsPiece* d_pieces, int64_t np, const hsdev::ConsBundle* d_bundles, const std::vector<hsdev::ConsBundle>& bundles,
                   const uint32_t* d_cig, int64_t traffic, int64_t extra_bytes, bool want_plan, const ConsPlanHook& before, const ConsPlanHook& after,
                   const std::function<std::string(int64_t)>& named, hipStream_t st, KernelClock& kc, BytesMoved& moved, ConsPlanStep& s) {
    using namespace hsdev;
    const int64_t nb = (int64_t)bundles.size();
    struct { int64_t plan, cols, recs, col_scan, rec_scan, tile_sum, ship; } w;
    WorkParts wp;
    w.plan = wp.take(np * (int64_t)sizeof(ConsPlan) + 16); w.cols = wp.take(np * 4 + 16); w.recs = wp.take(np * 4 + 16); w.col_scan = wp.take((np + 1) * 8 + 16);
    w.rec_scan = wp.take((np + 1) * 8 + 16); w.tile_sum = wp.take((int64_t)std::max(scan_tiles(np), 1) * 16);
    const int64_t extra_at = 16 + nb * (int64_t)sizeof(ConsBundlePlan), skip_at = extra_at + extra_bytes, ship_bytes = skip_at + nb * 4;
    w.ship = wp.take(ship_bytes + 16);
    if (int rc = s.work.alloc((size_t)wp.o)) return rc;
    char* work = (char*)s.work.p;
    ConsPlan* d_plan = (ConsPlan*)(work + w.plan);
    s.d_cols = (int32_t*)(work + w.cols); s.d_recs = (int32_t*)(work + w.recs); s.col_scan = (int64_t*)(work + w.col_scan); s.rec_scan = (int64_t*)(work + w.rec_scan);
    s.d_extra = work + w.ship + extra_at;
    EventPair ev;
    if (int rc = ev.take()) return rc;
    if (int rc = timed_launch(kc, ev, st, traffic, [&]() -> int {
            HS_HIP(hipMemsetAsync(work + w.ship, 0, (size_t)ship_bytes, st));
            HS_HIP(hipMemsetAsync(work + w.ship, 0x7f, 4, st));      // (first_long: no piece yet)
            if (before) { if (int rc = before(s)) return rc; }
            if (np) hipLaunchKernelGGL(k_cons_plan, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, st, d_pieces, (int)np, d_bundles, d_cig, d_plan, s.d_cols, s.d_recs,
                                       (ConsBundlePlan*)(work + w.ship + 16), (int32_t*)(work + w.ship + skip_at), (int32_t*)(work + w.ship));
            HS_HIP(hipGetLastError());
            if (int rc = exclusive_scan_launch(s.d_cols, (int)np, s.col_scan, (long long*)(work + w.tile_sum), st)) return rc;
            if (int rc = exclusive_scan_launch(s.d_recs, (int)np, s.rec_scan, (long long*)(work + w.tile_sum), st)) return rc;      // (it takes the tile scratch over: the stream orders it)
            return after ? after(s) : HS_OK; })) return rc;
    if (int rc = s.ship.alloc((size_t)ship_bytes + 16)) return rc;
    Shipment sh;
    sh.add(s.ship.p, work + w.ship, (size_t)ship_bytes);
    if (want_plan && np) {
        if (int rc = s.plan.alloc((size_t)np * sizeof(ConsPlan) + 16)) return rc;
        sh.add(s.plan.p, d_plan, (size_t)np * sizeof(ConsPlan));
    }
    if (int rc = sh.launch(st)) return rc;
    if (int rc = stream_wait(st)) return rc;      // the wait for the sizes
    kc.flush();
    (void)ev.ms(&s.ms);
    moved.down += ship_bytes + (want_plan ? np * (int64_t)sizeof(ConsPlan) : 0);
    const char* h = (const char*)s.ship.p;
    const int32_t first_long = *(const int32_t*)h;
    s.bplan = (const ConsBundlePlan*)(h + 16); s.extra = h + extra_at; s.bskip = (const int32_t*)(h + skip_at);
    if (first_long >= 0 && first_long < np) { set_error(std::string(who) + ": " + named(first_long) + ": a CIGAR of more than 2^31 - 1 bases"); return HS_EINVAL; }
    for (int64_t k = 0; k < nb; ++k) {
        const int64_t L = bundles[(size_t)k].L, n_own = bundles[(size_t)k].piece1 - bundles[(size_t)k].piece0;
        if (s.bplan[k].row_bytes < 0 || s.bplan[k].row_bytes > L * n_own || s.bplan[k].n_rec < 0 || s.bplan[k].n_rec > s.bplan[k].row_bytes || s.bskip[k] < 0 || s.bskip[k] > n_own) {
            set_error(std::string(who) + ": the device's plan does not fit the bundles");
            return HS_EHIP;
        }
    }
    return HS_OK;
}

// ---- the resident route: the bundles [b0, b1) of `in` whose bases, CIGAR words and backbones lie on the device (d_*: where the range begins;
// in.bases / in.cigar / in.backbone are not read). The host knows every offset, start, flag and base count, but not what a CIGAR sums to: the
// plan of every piece is the plan step's. Then sub-rounds of whole bundles within HS_CONSENSUS_CHUNK_MB, by the rule of
// consensus_device (cons_cut_round): k_cons_layout, then consensus_round_body (two waits each) or, with passes, refine_sub_round.
// H grows by the range's bundles (n_skipped included). plan_out (may be null): [4 * pieces of the range].
struct ConsResidentStats { int64_t n_sub_rounds = 0; double t_plan_ms = 0; double t_ms[4] = {0, 0, 0, 0}; BytesMoved moved; };
// the polishing passes of a sub-round (hs_capi_refine.inc, behind hs_capi_realign.inc: it takes the moves -> words route from there); their
// per-pass figures are summed straight into the block the C ABI returns
using RefineStats = hs_refined_result;
struct RefineSubRound {
    const hsdev::ConsPiece* d_src; const hsdev::ConsPiece* h_src; int64_t bundle_shift;      // the sub-round's pieces as k_cons_plan read them, on the device and on the host
    const std::vector<hsdev::ConsBundle>* bundles; const int32_t* n_skipped; int32_t* n_skipped_out;      // its bundles; pass 1's skipped pieces; where the last pass's go
    const uint8_t* d_bases; int64_t n_base;
};
int refine_sub_round(const char* who, const ConsRound& first, const RefineSubRound& sr, const hs_consensus_params& prm, hipStream_t st, KernelClock& kc, int32_t n_passes,
                     hs::ConsensusHost& H, ConsResidentStats& stats, RefineStats& rs);
// refine (null: one pass, as ever) / n_passes: the passes of every sub-round and where their figures go
int consensus_resident(const char* who, const ConsInput& in, int64_t b0, int64_t b1, const uint8_t* d_bases, const uint32_t* d_cig, const uint8_t* d_bb,
                       const hs_consensus_params& prm, hipStream_t st, hs::ConsensusHost& H, ConsResidentStats& stats, int32_t* plan_out, RefineStats* refine = nullptr,
                       int32_t n_passes = 1) {
    using namespace hsdev;
    const int64_t nb = b1 - b0, p0 = in.piece_off[b0], p1 = in.piece_off[b1], np = p1 - p0;
    if (nb <= 0) return HS_OK;
    const int64_t base0 = np ? in.base_off[p0] : 0, cig0 = np ? in.cig_off[p0] : 0, bb0 = in.backbone_off[b0];
    if (nb > 0x7fffffff - 256 || np > 0x7fffffff - 256) { set_error(std::string(who) + ": a round is too large; lower HS_POLISH_CHUNK_MB"); return HS_EINVAL; }
    std::vector<ConsPiece> pieces((size_t)np);
    std::vector<ConsBundle> bundles((size_t)nb);
    for (int64_t b = b0; b < b1; ++b) {
        const int64_t L = in.backbone_off[b + 1] - in.backbone_off[b], col_off = in.backbone_off[b] - bb0;
        bundles[(size_t)(b - b0)] = ConsBundle{col_off, (int32_t)(in.piece_off[b] - p0), (int32_t)(in.piece_off[b + 1] - p0), (int32_t)L, in.ovl[b], in.ovr[b], 0};
        for (int64_t p = in.piece_off[b]; p < in.piece_off[b + 1]; ++p) {
            if (in.sam[p] < 1) { set_error(std::string(who) + ": piece " + std::to_string(p) + ": a start position below 1"); return HS_EINVAL; }
            // (what k_cons_plan reads of a piece: its bundle in row_off, its base count in n_cols, its flags in n_rec)
            pieces[(size_t)(p - p0)] = ConsPiece{in.base_off[p] - base0, in.cig_off[p] - cig0, b - b0, 0, col_off, (int32_t)(in.cig_off[p + 1] - in.cig_off[p]), in.sam[p] - 1,
                                                 (int32_t)(in.base_off[p + 1] - in.base_off[p]), in.flags[p]};
        }
    }
    // ---- the plan
    DBuf d_pieces, d_bundles;
    UploadPack pk;
    pk.add(pieces, d_pieces); pk.add(bundles, d_bundles);
    stats.moved.up += (int64_t)pk.total;
    if (int rc = pk.commit(st)) return rc;
    KernelClock kc;
    ConsPlanStep plan;
    if (int rc = cons_plan_step(who, d_pieces.as<ConsPiece>(), np, d_bundles.as<ConsBundle>(), bundles, d_cig, (in.cig_off[p1] - cig0) * 4 + np * (int64_t)(sizeof(ConsPiece) + sizeof(ConsPlan) + 8),
                                0, plan_out != nullptr, nullptr, nullptr, [&](int64_t piece) {
                                    int64_t b = b0;
                                    while (b + 1 < b1 && in.piece_off[b + 1] <= p0 + piece) ++b;
                                    return "bundle " + std::to_string(b); },
                                st, kc, stats.moved, plan)) return rc;
    stats.t_plan_ms += plan.ms;
    if (plan_out && np) std::memcpy(plan_out, plan.plan.p, (size_t)np * sizeof(ConsPlan));
    std::vector<ConsBundleSize> sizes((size_t)nb);
    for (int64_t k = 0; k < nb; ++k) sizes[(size_t)k] = ConsBundleSize{plan.bplan[k].row_bytes, plan.bplan[k].n_rec, bundles[(size_t)k].L};
    H.n_skipped.insert(H.n_skipped.end(), plan.bskip, plan.bskip + nb);
    const size_t skipped_at = H.n_skipped.size() - (size_t)nb;

    // ---- sub-rounds of whole bundles
    ConsCut cut;
    for (int64_t s0 = 0; s0 < nb; s0 = cut.s1) {
        if (int rc = cons_cut_round(who, sizes, b0, s0, cut)) return rc;
        ++stats.n_sub_rounds;
        const int64_t s1 = cut.s1, q0 = bundles[(size_t)s0].piece0, q1 = bundles[(size_t)(s1 - 1)].piece1, nq = q1 - q0, col0 = bundles[(size_t)s0].col_off;
        const int64_t sbase0 = nq ? pieces[(size_t)q0].base_off : 0, scig0 = nq ? pieces[(size_t)q0].cig_off : 0;
        const int64_t sbase1 = q1 < np ? pieces[(size_t)q1].base_off : (np ? in.base_off[p1] - base0 : 0), scig1 = q1 < np ? pieces[(size_t)q1].cig_off : (np ? in.cig_off[p1] - cig0 : 0);
        std::vector<ConsBundle> sb;
        std::vector<ConsTile> tiles;
        if (int rc = cons_round_tables(who, s1 - s0, cut.n_rec, [&](int64_t k) {
                ConsBundle b = bundles[(size_t)(s0 + k)];
                b.col_off -= col0; b.piece0 -= (int32_t)q0; b.piece1 -= (int32_t)q0;
                return b; }, sb, tiles)) return rc;
        DBuf d_sb, d_tiles, d_sp;
        UploadPack spk;
        spk.add(sb, d_sb); spk.add(tiles, d_tiles);
        stats.moved.up += (int64_t)spk.total;
        if (int rc = spk.commit(st)) return rc;
        if (int rc = d_sp.alloc((size_t)std::max<int64_t>(nq, 1) * sizeof(ConsPiece))) return rc;
        EventPair ev_lay;
        if (int rc = ev_lay.take()) return rc;
        if (int rc = timed_launch(kc, ev_lay, st, nq * (int64_t)(2 * sizeof(ConsPiece) + 24), [&]() -> int {
                if (nq) hipLaunchKernelGGL(k_cons_layout, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_pieces.as<ConsPiece>(), (long long)q0, (int)nq, plan.d_cols, plan.d_recs,
                                           plan.col_scan, plan.rec_scan, (long long)sbase0, (long long)scig0, (long long)col0, d_sp.as<ConsPiece>());
                HS_HIP(hipGetLastError());
                return HS_OK; })) return rc;
        const ConsRound round{d_bases + sbase0, d_cig + scig0, d_bb + col0, d_sp.as<ConsPiece>(), d_sb.as<ConsBundle>(), d_tiles.as<ConsTile>(),
                              nq, s1 - s0, (int64_t)tiles.size(), cut.rb, cut.n_rec, cut.C, sbase1 - sbase0, scig1 - scig0};
        if (refine && n_passes > 1) {
            const RefineSubRound sr{d_pieces.as<ConsPiece>() + q0, pieces.data() + q0, s0, &sb, plan.bskip + s0, H.n_skipped.data() + skipped_at + s0, d_bases + sbase0, sbase1 - sbase0};
            if (int rc = refine_sub_round(who, round, sr, prm, st, kc, n_passes, H, stats, *refine)) return rc;
        } else if (int rc = consensus_round_body(who, round, prm, st, kc, stats.t_ms, H, &stats.moved)) return rc;
        { float ms = 0; if (ev_lay.ms(&ms) == HS_OK) stats.t_plan_ms += ms; }
    }
    return HS_OK;
}

// the arrays of consensus_device, checked as it checks them and uploaded whole, then the resident route: one pass through consensus_round_body
// (refine null), more through refine_sub_round. stats (may be null): the route's figures for a caller that reports them
int consensus_arrays_resident(const char* who, const ConsInput& given, const hs_consensus_params& prm, int32_t* plan_out, hs_consensus_result** out, ConsResidentStats* stats_out = nullptr,
                              RefineStats* refine = nullptr, int32_t n_passes = 1) {
    ConsInput in;
    if (int rc = cons_input_checked(who, given, prm, in)) return rc;
    const int64_t nb = in.n_bundles, np = in.piece_off[nb];
    DBuf d_bases, d_cigar, d_bb;
    if (int rc = upload_pageable(d_bases, in.bases, (size_t)in.base_off[np], 0, 16)) return rc;
    if (int rc = upload_pageable(d_cigar, in.cigar, (size_t)in.cig_off[np] * 4, 0, 16)) return rc;
    if (int rc = upload_pageable(d_bb, in.backbone, (size_t)in.backbone_off[nb], 0, 16)) return rc;
    hs::ConsensusHost H;
    H.cons_off.assign(1, 0);
    ConsResidentStats stats;
    if (int rc = consensus_resident(who, in, 0, nb, d_bases.as<uint8_t>(), d_cigar.as<uint32_t>(), d_bb.as<uint8_t>(), prm, nullptr, H, stats, plan_out, refine, n_passes)) return rc;
    if (stats_out) *stats_out = stats;
    *out = cons_result_finish(who, H, stats.t_ms, stats.n_sub_rounds);
    return *out ? HS_OK : HS_EINVAL;
}

// ---- from labels to haplotype sequences: hs_polish_inputs' rounds with the consensus as their sink
int haplotypes_core(const char* who, hs_cv_batch* b, int c0, int c1, const std::vector<std::vector<hs::LabelledInterval>>& ivs, const std::vector<uint8_t>& has,
                    bool polish_everything, const hs_consensus_params& prm, BytesMoved moved, hs_haplotypes_result** out, RefineStats* refine = nullptr, int32_t n_passes = 1) {
    hs::ConsensusHost H;
    H.cons_off.assign(1, 0);
    ConsResidentStats stats;
    stats.moved = moved;
    const PolishSink sink = [&](const PolishRound& r) -> int {
        const ConsInput in{r.b1, r.backbone_off, nullptr, r.ovl, r.ovr, r.piece_off, r.sam, r.flags, r.base_off, nullptr, r.cig_off, nullptr};
        return consensus_resident(who, in, r.b0, r.b1, r.d_bases, r.d_cig, r.d_bb, prm, r.st, H, stats, nullptr, refine, n_passes);
    };
    hs_polish_result* inputs = nullptr;
    if (int rc = polish_inputs_core(b, c0, c1, ivs, has, polish_everything, &inputs, &sink, &stats.moved)) return rc;
    std::unique_ptr<hs_polish_result, void (*)(hs_polish_result*)> iguard(inputs, hs_polish_result_destroy);
    hs_consensus_result* cons = cons_result_finish(who, H, stats.t_ms, stats.n_sub_rounds);
    hs_haplotypes_result* res = static_cast<hs_haplotypes_result*>(std::calloc(1, sizeof(hs_haplotypes_result)));
    if (!cons || !res) { hs_consensus_result_destroy(cons); std::free(res); set_error(std::string(who) + ": out of host memory"); return HS_EINVAL; }
    res->inputs = iguard.release(); res->consensus = cons;
    res->n_rounds = inputs->n_rounds; res->n_sub_rounds = stats.n_sub_rounds; res->bytes_down = stats.moved.down; res->bytes_up = stats.moved.up; res->t_plan_ms = stats.t_plan_ms;
    *out = res;
    return HS_OK;
}

// the one body of hs_polish_haplotypes and hs_polish_haplotypes_refined (refine null: one pass): the labels into intervals, then haplotypes_core
int haplotypes_labels(const char* who, hs_cv_batch* b, int32_t c0, int32_t c1, const int64_t* win_off, const int32_t* win_start, const int32_t* win_end, const int64_t* label_off,
                      const int32_t* labels, const uint8_t* contig_has_snps, int32_t polish_everything, const hs_consensus_params* params, hs_haplotypes_result** out,
                      RefineStats* refine, int32_t n_passes) {
    if (!b || !out || !win_off || !label_off || c0 < 0 || c1 < c0 || c1 > b->n_contigs) { set_error(std::string(who) + ": bad arguments"); return HS_EINVAL; }
    *out = nullptr;
    const hs_consensus_params prm = params ? *params : hs_consensus_default_params();
    if (!hs::consensus_params_valid(prm)) { set_error(std::string(who) + ": parameters out of range (min_cov >= 1, max_ins 1..64)"); return HS_EINVAL; }
    if (int rc = bind_device(b->device)) return rc;
    try {
        BytesMoved moved;
        if (int rc = polish_host_recs(b, &moved)) return rc;
        std::vector<std::vector<hs::LabelledInterval>> ivs;
        std::vector<uint8_t> has;
        if (int rc = hs::polish_intervals_from_labels(b->n_contigs, b->contig_rec_off.data(), b->h_rec_read.data(), win_off, win_start, win_end, label_off, labels,
                                                      contig_has_snps, ivs, has))
            return rc;
        return haplotypes_core(who, b, c0, c1, ivs, has, polish_everything != 0, prm, moved, out, refine, n_passes);
    } catch (const std::exception& e) { set_error(std::string(who) + ": " + e.what()); return HS_EINVAL; }
}

}  // namespace

extern "C" {

void hs_haplotypes_result_destroy(hs_haplotypes_result* r) {
    if (!r) return;
    hs_polish_result_destroy(r->inputs);
    hs_consensus_result_destroy(r->consensus);
    std::free(r);
}

int hs_polish_haplotypes(hs_cv_batch* b, int32_t c0, int32_t c1, const int64_t* win_off, const int32_t* win_start, const int32_t* win_end, const int64_t* label_off,
                         const int32_t* labels, const uint8_t* contig_has_snps, int32_t polish_everything, const hs_consensus_params* params, hs_haplotypes_result** out) {
    if (int rc = require_device()) return rc;
    return haplotypes_labels("hs_polish_haplotypes", b, c0, c1, win_off, win_start, win_end, label_off, labels, contig_has_snps, polish_everything, params, out, nullptr, 1);
}

// the one body of hs_polish_haplotypes_from_files and hs_polish_haplotypes_refined_from_files (refine null: one pass)
static int haplotypes_files(const char* who_c, const char* gfa, const char* reads, const char* sam, const char* gro, int32_t polish_everything, const hs_consensus_params* params,
                            const char* out_fasta, int32_t n_threads, RefineStats* refine, int32_t n_passes) {
    const std::string who(who_c);
    if (int rc = require_device()) return rc;
    if (!gfa || !reads || !sam || !gro || !out_fasta) { set_error(who + ": null path"); return HS_EINVAL; }
    const hs_consensus_params prm = params ? *params : hs_consensus_default_params();
    if (!hs::consensus_params_valid(prm)) { set_error(who + ": parameters out of range (min_cov >= 1, max_ins 1..64)"); return HS_EINVAL; }
    try {
        hs::CvFileInput in;
        if (int rc = hs::load_cv_inputs(gfa, reads, sam, false, in, n_threads < 1 ? 1 : n_threads)) return rc;
        std::vector<std::vector<hs::LabelledInterval>> ivs;
        std::vector<uint8_t> has;
        if (int rc = hs::polish_intervals_from_gro(in, gro, ivs, has)) return rc;
        const int32_t n_contigs = (int32_t)in.contig_names.size();
        hs_cv_batch* b = nullptr;
        if (int rc = hs_cv_batch_create(in.contig_seq.data(), in.contig_off.data(), n_contigs, in.read_seq.data(), in.read_off.data(), (int32_t)in.read_names.size(),
                                        in.rec_read.data(), in.rec_pos.data(), in.rec_strand.data(), in.rec_cig_off.data(), in.cigar.data(), in.contig_rec_off.data(), &b))
            return rc;
        std::unique_ptr<hs_cv_batch, void (*)(hs_cv_batch*)> bguard(b, hs_cv_batch_destroy);
        hs_haplotypes_result* r = nullptr;
        if (int rc = haplotypes_core(who_c, b, 0, n_contigs, ivs, has, polish_everything != 0, prm, BytesMoved(), &r, refine, n_passes)) return rc;
        std::unique_ptr<hs_haplotypes_result, void (*)(hs_haplotypes_result*)> rguard(r, hs_haplotypes_result_destroy);
        std::FILE* f = std::fopen(out_fasta, "wb");
        if (!f) { set_error(std::string("cannot write ") + out_fasta); return HS_EIO; }
        std::string text;
        bool ok = true;
        const hs_polish_result* pi = r->inputs;
        const hs_consensus_result* co = r->consensus;
        for (int64_t k = 0; k < pi->n_bundles && ok; ++k) {
            text.clear();
            hs::haplotype_fasta_record(in.contig_names[(size_t)pi->bundle_contig[k]], pi->bundle_start[k], pi->bundle_end[k], pi->bundle_group[k], co->cons + co->cons_off[k],
                                       co->cons_off[k + 1] - co->cons_off[k], co->trim_start[k], co->trim_end[k], text);
            ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
        }
        ok = std::fclose(f) == 0 && ok;
        if (!ok) { set_error(std::string("short write on ") + out_fasta); return HS_EIO; }
        return HS_OK;
    } catch (const std::exception& e) { set_error(who + ": " + e.what()); return HS_EINVAL; }
}

int hs_polish_haplotypes_from_files(const char* gfa, const char* reads, const char* sam, const char* gro, int32_t polish_everything, const hs_consensus_params* params,
                                    const char* out_fasta, int32_t n_threads) {
    return haplotypes_files("hs_polish_haplotypes_from_files", gfa, reads, sam, gro, polish_everything, params, out_fasta, n_threads, nullptr, 1);
}

int hs_polish_consensus_planned_tap(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                                    const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                                    const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params* params, int32_t* plan_out, hs_consensus_result** out) {
    if (int rc = require_device()) return rc;
    if (!out) { set_error("hs_polish_consensus_planned_tap: bad arguments"); return HS_EINVAL; }
    *out = nullptr;
    const ConsInput in{n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar};
    try { return consensus_arrays_resident("hs_polish_consensus_planned_tap", in, params ? *params : hs_consensus_default_params(), plan_out, out); }
    catch (const std::exception& e) { set_error(std::string("hs_polish_consensus_planned_tap: ") + e.what()); return HS_EINVAL; }
}

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
