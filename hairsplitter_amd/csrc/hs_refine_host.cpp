// hs_refine_host.cpp -- the host half of the polishing passes (hs_refine_host.h): one pass of the consensus on the host with the column figures
// and every piece's window in its text. No device code and no HIP call.
#include "hs_refine_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace hs {

int refine_plan_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                     const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                     const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, int n_threads, RefinePlanHost& out, std::string& err) {
    out = RefinePlanHost();
    if (int rc = consensus_host_columns(n_bundles, backbone_off, backbone, overhang_left, overhang_right, piece_off, piece_sam_pos, piece_flags, base_off, bases, cig_off, cigar,
                                        prm, n_threads, out.cons, &out.cols, err))
        return rc;
    const int64_t n_pieces = piece_off[n_bundles];
    out.win_start.assign((size_t)n_pieces, -1); out.win_end.assign((size_t)n_pieces, -1);
    for (int64_t b = 0; b < n_bundles; ++b) {
        const int64_t L = backbone_off[b + 1] - backbone_off[b];
        const int32_t* begin = out.cols.col_begin.data() + out.cols.col_off[(size_t)b];
        const int32_t* ins = out.cols.col_ins.data() + out.cols.col_off[(size_t)b];
        for (int64_t p = piece_off[b]; p < piece_off[b + 1]; ++p) {
            const ConsPiecePlan pl = cons_piece_plan(cigar + cig_off[p], cig_off[p + 1] - cig_off[p], base_off[p + 1] - base_off[p], piece_flags[p], piece_sam_pos[p], L);
            if (!refine_has_window(pl.skipped, pl.n_cols)) continue;
            const int64_t s0 = (int64_t)piece_sam_pos[p] - 1;
            refine_window(begin[s0], ins[s0], begin[s0 + pl.n_cols], &out.win_start[(size_t)p], &out.win_end[(size_t)p]);
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

hs_refine_plan* refine_plan_from_host(const RefinePlanHost& h) {
    hs_refine_plan* r = static_cast<hs_refine_plan*>(std::calloc(1, sizeof(hs_refine_plan)));
    if (!r) return nullptr;
    r->consensus = consensus_result_from_host(h.cons);
    r->n_bundles = (int64_t)h.cols.col_off.size() - 1; r->n_pieces = (int64_t)h.win_start.size();
    r->col_off = malloc_vec(h.cols.col_off); r->col_begin = malloc_vec(h.cols.col_begin); r->col_ins = malloc_vec(h.cols.col_ins);
    r->win_start = malloc_vec(h.win_start); r->win_end = malloc_vec(h.win_end);
    if (!r->consensus || !r->col_off || !r->col_begin || !r->col_ins || !r->win_start || !r->win_end) { hs_refine_plan_destroy(r); return nullptr; }
    return r;
}

}  // namespace hs

extern "C" {

void hs_refine_plan_destroy(hs_refine_plan* r) {
    if (!r) return;
    hs_consensus_result_destroy(r->consensus);
    void* p[] = {r->col_off, r->col_begin, r->col_ins, r->win_start, r->win_end};
    for (void* q : p) std::free(q);
    std::free(r);
}

}  // extern "C"
