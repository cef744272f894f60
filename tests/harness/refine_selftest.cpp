// TEST INFRASTRUCTURE: the device-free half of the polishing passes (hs_refine_host.h / .cpp on hs_consensus_host.cpp) as a program of its own, for
// tests/test_cpu_refine.py to hold against the numpy form of tests/refine_cases.py.
// argv[1]: a text file written by consensus_cases.write_job (the format of consensus_selftest.cpp).
// stdout: per bundle "C <bundle> <trim_start> <trim_end> <n_sub> <n_del> <n_ins_bases> <n_low> <n_skipped> <consensus | ->", then
//   "K <bundle> <n = L + 1> <col_begin x n> <col_ins x n>", then "N <bundle> <next overhang_left> <next overhang_right>", and per piece
//   "W <piece> <win_start> <win_end> <next piece_sam_pos> <the word of an empty window | 0>". Exit 4: the call is refused.
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../hairsplitter_amd/csrc/hs_refine_host.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: refine_selftest <job.txt>\n"); return 2; }
    std::ifstream f(argv[1]);
    hs_consensus_params prm;
    int threads = 1;
    int64_t n_bundles = 0;
    if (!(f >> prm.min_cov >> prm.max_ins >> threads >> n_bundles) || n_bundles < 0) { std::fprintf(stderr, "refine_selftest: bad header\n"); return 2; }
    std::vector<int64_t> bb_off{0}, piece_off{0}, base_off{0}, cig_off{0};
    std::vector<uint8_t> bb, bases;
    std::vector<int32_t> ovl, ovr, sam, flags;
    std::vector<uint32_t> cigar;
    for (int64_t b = 0; b < n_bundles; ++b) {
        std::string tag, text;
        int32_t l = 0, r = 0;
        int64_t np = 0;
        if (!(f >> tag >> l >> r >> np >> text) || tag != "B" || np < 0) { std::fprintf(stderr, "refine_selftest: bad bundle line\n"); return 2; }
        if (text != "-") bb.insert(bb.end(), text.begin(), text.end());
        bb_off.push_back((int64_t)bb.size()); ovl.push_back(l); ovr.push_back(r);
        for (int64_t p = 0; p < np; ++p) {
            int32_t s = 0, fl = 0;
            int64_t nw = 0;
            if (!(f >> tag >> s >> fl >> nw) || tag != "P" || nw < 0) { std::fprintf(stderr, "refine_selftest: bad piece line\n"); return 2; }
            for (int64_t i = 0; i < nw; ++i) { uint32_t w = 0; if (!(f >> w)) return 2; cigar.push_back(w); }
            if (!(f >> text)) return 2;
            if (text != "-") bases.insert(bases.end(), text.begin(), text.end());
            sam.push_back(s); flags.push_back(fl); base_off.push_back((int64_t)bases.size()); cig_off.push_back((int64_t)cigar.size());
        }
        piece_off.push_back((int64_t)sam.size());
    }
    hs::RefinePlanHost out;
    std::string err;
    if (int rc = hs::refine_plan_host(n_bundles, bb_off.data(), bb.data(), ovl.data(), ovr.data(), piece_off.data(), sam.data(), flags.data(), base_off.data(), bases.data(),
                                      cig_off.data(), cigar.data(), prm, threads, out, err)) {
        std::fprintf(stderr, "refine_selftest: %s\n", err.c_str());
        return rc == HS_EINVAL ? 4 : 3;
    }
    // through the malloc'd form and back, so that it is exercised too
    hs_refine_plan* r = hs::refine_plan_from_host(out);
    if (!r) return 3;
    const hs_consensus_result* c = r->consensus;
    for (int64_t b = 0; b < n_bundles; ++b) {
        std::printf("C %lld %d %d %d %d %d %d %d ", (long long)b, c->trim_start[b], c->trim_end[b], c->n_sub[b], c->n_del[b], c->n_ins_bases[b], c->n_low[b], c->n_skipped[b]);
        if (c->cons_off[b + 1] == c->cons_off[b]) std::fputs("-", stdout);
        else std::fwrite(c->cons + c->cons_off[b], 1, (size_t)(c->cons_off[b + 1] - c->cons_off[b]), stdout);
        std::fputc('\n', stdout);
        const int64_t n = r->col_off[b + 1] - r->col_off[b];
        std::printf("K %lld %lld", (long long)b, (long long)n);
        for (int64_t t = 0; t < n; ++t) std::printf(" %d", r->col_begin[r->col_off[b] + t]);
        for (int64_t t = 0; t < n; ++t) std::printf(" %d", r->col_ins[r->col_off[b] + t]);
        std::fputc('\n', stdout);
        std::printf("N %lld %d %d\n", (long long)b, hs::refine_overhang_left(c->trim_start[b]), hs::refine_overhang_right(c->cons_off[b + 1] - c->cons_off[b], c->trim_end[b]));
    }
    for (int64_t p = 0; p < r->n_pieces; ++p) {
        const bool empty = r->win_start[p] >= 0 && r->win_end[p] == r->win_start[p];
        std::printf("W %lld %lld %lld %d %u\n", (long long)p, (long long)r->win_start[p], (long long)r->win_end[p], hs::refine_sam_pos(r->win_start[p]),
                    empty ? hs::refine_empty_word(base_off[p + 1] - base_off[p]) : 0u);
    }
    hs_refine_plan_destroy(r);
    return 0;
}
