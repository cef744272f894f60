// hs_consensus_host.cpp -- the host half of the bundle consensus (hs_consensus_host.h): a whole call on the host's threads, ending in the
// rule functions the kernels end in. No device code and no HIP call.
#include "hs_consensus_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace hs {

int consensus_check(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                    const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                    const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, std::string& err) {
    if (!consensus_params_valid(prm)) { err = "parameters out of range (min_cov >= 1, max_ins 1..64)"; return HS_EINVAL; }
    if (n_bundles < 0 || !backbone_off || !piece_off || (n_bundles > 0 && (!overhang_left || !overhang_right))) { err = "bad arguments"; return HS_EINVAL; }
    if (backbone_off[0] != 0 || piece_off[0] != 0) { err = "offsets do not begin at 0"; return HS_EINVAL; }
    for (int64_t b = 0; b < n_bundles; ++b) {
        const int64_t L = backbone_off[b + 1] - backbone_off[b];
        if (L < 0 || L > 0x7fffffff - 256 || piece_off[b + 1] < piece_off[b]) { err = "bundle " + std::to_string(b) + ": descending offsets or a backbone beyond 2^31"; return HS_EINVAL; }
        if (overhang_left[b] < 0 || overhang_right[b] < 0) { err = "bundle " + std::to_string(b) + ": a negative overhang"; return HS_EINVAL; }
    }
    const int64_t n_pieces = piece_off[n_bundles];
    if (backbone_off[n_bundles] > 0 && !backbone) { err = "bad arguments"; return HS_EINVAL; }
    if (n_pieces > 0x7fffffff - 256) { err = "more than 2^31 pieces in one call"; return HS_EINVAL; }
    if (n_pieces > 0 && (!piece_sam_pos || !piece_flags || !base_off || !cig_off || base_off[0] != 0 || cig_off[0] != 0)) { err = "bad arguments"; return HS_EINVAL; }
    for (int64_t p = 0; p < n_pieces; ++p) {
        if (base_off[p + 1] < base_off[p] || cig_off[p + 1] < cig_off[p]) { err = "piece " + std::to_string(p) + ": descending offsets"; return HS_EINVAL; }
        if (piece_sam_pos[p] < 1) { err = "piece " + std::to_string(p) + ": a start position below 1"; return HS_EINVAL; }
    }
    if (n_pieces > 0 && ((base_off[n_pieces] > 0 && !bases) || (cig_off[n_pieces] > 0 && !cigar))) { err = "bad arguments"; return HS_EINVAL; }
    return HS_OK;
}

namespace {

struct BundleOut { std::vector<uint8_t> text; int32_t v[7]; int64_t n_rec, n_slots; bool long_cigar; bool want_cols = false; std::vector<int32_t> col_begin, col_ins; };

// one bundle, by the rule: the walk of every piece into per-column counters and per-slot lists of insertions, then the decisions
void consensus_bundle(int64_t L, const uint8_t* B, int32_t ovl, int32_t ovr, int64_t p0, int64_t p1, const int32_t* sam, const int32_t* flags, const int64_t* base_off,
                      const uint8_t* bases, const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, BundleOut& o) {
    struct Ins { int64_t slot, src; int32_t len; };
    std::vector<uint32_t> votes((size_t)L * 5, 0), nins((size_t)L, 0), span((size_t)L, 0);
    std::vector<Ins> ins;
    int32_t n_skipped = 0;
    o.long_cigar = false;
    for (int64_t p = p0; p < p1; ++p) {
        const uint32_t* cg = cigar + cig_off[p];
        const int64_t n_ops = cig_off[p + 1] - cig_off[p], n_bases = base_off[p + 1] - base_off[p];
        const ConsPiecePlan plan = cons_piece_plan(cg, n_ops, n_bases, flags[p], sam[p], L);
        if (plan.long_cigar) { o.long_cigar = true; return; }
        if (plan.skipped) { ++n_skipped; continue; }
        const uint8_t* P = bases + base_off[p];
        int64_t t = (int64_t)sam[p] - 1, q = 0, pending = 0, pending_src = 0;
        bool covered_prev = false;
        for (int64_t i = 0; i < n_ops && t < L; ++i) {
            const uint32_t c = cg[i] & 15u;
            const int64_t len = (int64_t)(cg[i] >> 4);
            if (c == 1) { if (pending == 0) pending_src = q; pending += len; q += len; continue; }
            if (c != 0 && c != 2) continue;
            for (int64_t e = 0; e < len && t < L; ++e, ++t) {
                votes[(size_t)t * 5 + (c == 0 ? cons_code(P[q + e]) : CONS_DEL)]++;
                if (covered_prev) {
                    span[(size_t)t]++;
                    if (pending > 0) { nins[(size_t)t]++; ins.push_back(Ins{t, base_off[p] + pending_src, cons_ins_cap(pending, prm.max_ins)}); }
                }
                pending = 0;
                covered_prev = true;
            }
            if (c == 0) q += len;
        }
    }
    // the slots that win, their tables
    std::vector<int64_t> slot_index((size_t)L, -1);
    int64_t n_slots = 0;
    for (int64_t t = 1; t < L; ++t) if (cons_slot_wins(nins[(size_t)t], span[(size_t)t], prm.min_cov)) slot_index[(size_t)t] = n_slots++;
    const int32_t W = cons_table_words(prm.max_ins);
    std::vector<uint32_t> tab((size_t)n_slots * W, 0);
    for (const Ins& x : ins) {
        if (slot_index[(size_t)x.slot] < 0) continue;
        uint32_t* t = &tab[(size_t)slot_index[(size_t)x.slot] * W];
        t[x.len]++;
        for (int32_t j = 0; j < x.len; ++j) t[prm.max_ins + 1 + 4 * j + cons_code(bases[x.src + j])]++;
    }
    int32_t n_sub = 0, n_del = 0, n_ib = 0, n_low = 0;
    const int64_t c_start = std::min<int64_t>(ovl, L), c_end = L - std::min<int64_t>(ovr, L);
    int32_t trim_start = 0, trim_end = 0;
    o.text.clear();
    if (o.want_cols) { o.col_begin.assign((size_t)L + 1, 0); o.col_ins.assign((size_t)L + 1, 0); }
    for (int64_t t = 0; t < L; ++t) {
        if (t == c_start) trim_start = (int32_t)o.text.size();
        if (t == c_end) trim_end = (int32_t)o.text.size();
        if (o.want_cols) o.col_begin[(size_t)t] = (int32_t)o.text.size();
        if (slot_index[(size_t)t] >= 0) {
            const uint32_t* tb = &tab[(size_t)slot_index[(size_t)t] * W];
            const int32_t l = cons_ins_length(tb, prm.max_ins);
            for (int32_t j = 0; j < l; ++j) o.text.push_back(cons_letter(cons_ins_base(tb, prm.max_ins, j)));
            n_ib += l;
            if (o.want_cols) o.col_ins[(size_t)t] = l;
        }
        const uint8_t cb = cons_column_byte(&votes[(size_t)t * 5], B[t], prm.min_cov);
        const int w = cb & CONS_COL_CODE;
        if (w == CONS_KEEP) { ++n_low; o.text.push_back(B[t]); }
        else if (w == CONS_DEL) ++n_del;
        else { o.text.push_back(cons_letter(w)); if (cb & CONS_COL_SUB) ++n_sub; }
    }
    if (o.want_cols) o.col_begin[(size_t)L] = (int32_t)o.text.size();
    if (c_start == L) trim_start = (int32_t)o.text.size();
    if (c_end == L) trim_end = (int32_t)o.text.size();
    const int32_t v[7] = {trim_start, trim_end, n_sub, n_del, n_ib, n_low, n_skipped};
    std::memcpy(o.v, v, sizeof v);
    o.n_rec = (int64_t)ins.size(); o.n_slots = n_slots;
}

}  // namespace

int consensus_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                   const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                   const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, int n_threads, ConsensusHost& out, std::string& err) {
    return consensus_host_columns(n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar, prm,
                                  n_threads, out, nullptr, err);
}

int consensus_host_columns(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                           const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                           const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, int n_threads, ConsensusHost& out, ConsensusColumns* cols,
                           std::string& err) {
    if (int rc = consensus_check(n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar, prm, err))
        return rc;
    std::vector<BundleOut> bo((size_t)n_bundles);
    if (cols) { *cols = ConsensusColumns(); cols->col_off.assign(1, 0); for (BundleOut& o : bo) o.want_cols = true; }
    n_threads = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, n_bundles));
    auto work = [&](int t) {
        for (int64_t b = t; b < n_bundles; b += n_threads)
            consensus_bundle(backbone_off[b + 1] - backbone_off[b], backbone + backbone_off[b], overhang_left[b], overhang_right[b], piece_off[b], piece_off[b + 1], piece_sam_pos,
                             piece_flags, base_off, bases, cig_off, cigar, prm, bo[(size_t)b]);
    };
    if (n_threads == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads; ++t) th.emplace_back(work, t);
        for (std::thread& t : th) t.join();
    }
    out = ConsensusHost();
    out.cons_off.assign(1, 0);
    std::vector<int32_t>* f[7] = {&out.trim_start, &out.trim_end, &out.n_sub, &out.n_del, &out.n_ins_bases, &out.n_low, &out.n_skipped};
    for (int64_t b = 0; b < n_bundles; ++b) {
        const BundleOut& o = bo[(size_t)b];
        if (o.long_cigar) { err = "bundle " + std::to_string(b) + ": a CIGAR of more than 2^31 - 1 bases"; return HS_EINVAL; }
        out.cons.insert(out.cons.end(), o.text.begin(), o.text.end());
        out.cons_off.push_back((int64_t)out.cons.size());
        for (int j = 0; j < 7; ++j) f[j]->push_back(o.v[j]);
        out.n_ins_records += o.n_rec; out.n_ins_slots += o.n_slots;
        if (cols) {
            cols->col_begin.insert(cols->col_begin.end(), o.col_begin.begin(), o.col_begin.end());
            cols->col_ins.insert(cols->col_ins.end(), o.col_ins.begin(), o.col_ins.end());
            cols->col_off.push_back((int64_t)cols->col_begin.size());
        }
    }
    return HS_OK;
}

namespace {
template <class T> T* malloc_vec(const std::vector<T>& v) {
    T* p = static_cast<T*>(std::malloc(std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
}  // namespace

hs_consensus_result* consensus_result_from_host(const ConsensusHost& h) {
    hs_consensus_result* r = static_cast<hs_consensus_result*>(std::calloc(1, sizeof(hs_consensus_result)));
    if (!r) return nullptr;
    r->n_bundles = (int64_t)h.cons_off.size() - 1;
    r->cons_off = malloc_vec(h.cons_off); r->cons = malloc_vec(h.cons);
    r->trim_start = malloc_vec(h.trim_start); r->trim_end = malloc_vec(h.trim_end); r->n_sub = malloc_vec(h.n_sub); r->n_del = malloc_vec(h.n_del);
    r->n_ins_bases = malloc_vec(h.n_ins_bases); r->n_low = malloc_vec(h.n_low); r->n_skipped = malloc_vec(h.n_skipped);
    r->n_ins_records = h.n_ins_records; r->n_ins_slots = h.n_ins_slots;
    if (!r->cons_off || !r->cons || !r->trim_start || !r->trim_end || !r->n_sub || !r->n_del || !r->n_ins_bases || !r->n_low || !r->n_skipped) {
        hs_consensus_result_destroy(r);
        return nullptr;
    }
    return r;
}

}  // namespace hs

extern "C" {

hs_consensus_params hs_consensus_default_params(void) { return hs_consensus_params{3, 32}; }

void hs_consensus_result_destroy(hs_consensus_result* r) {
    if (!r) return;
    void* p[] = {r->cons_off, r->cons, r->trim_start, r->trim_end, r->n_sub, r->n_del, r->n_ins_bases, r->n_low, r->n_skipped};
    for (void* q : p) std::free(q);
    std::free(r);
}

}  // extern "C"
