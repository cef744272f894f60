// TEST INFRASTRUCTURE: the device-free half of the bundle consensus (hs_consensus_host.h / .cpp -- the rule functions the kernels end in, and the
// whole call on the host) as a program of its own, for tests/test_cpu_consensus.py to hold against the numpy form of tests/consensus_cases.py.
// argv[1]: a text file written by consensus_cases.write_job:
//   min_cov max_ins threads
//   n_bundles, then per bundle a line "B <overhang_left> <overhang_right> <n_pieces> <backbone | ->" and per piece a line
//   "P <sam_pos> <flags> <n_words> <word> ... <bases | ->" ("-": empty)
// stdout: per bundle "C <bundle> <trim_start> <trim_end> <n_sub> <n_del> <n_ins_bases> <n_low> <n_skipped> <consensus | ->", then
// "T <n_ins_records> <n_ins_slots>". Exit 4: the call is refused.
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../hairsplitter_amd/csrc/hs_consensus_host.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: consensus_selftest <job.txt>\n"); return 2; }
    std::ifstream f(argv[1]);
    hs_consensus_params prm;
    int threads = 1;
    int64_t n_bundles = 0;
    if (!(f >> prm.min_cov >> prm.max_ins >> threads >> n_bundles) || n_bundles < 0) { std::fprintf(stderr, "consensus_selftest: bad header\n"); return 2; }
    std::vector<int64_t> bb_off{0}, piece_off{0}, base_off{0}, cig_off{0};
    std::vector<uint8_t> bb, bases;
    std::vector<int32_t> ovl, ovr, sam, flags;
    std::vector<uint32_t> cigar;
    for (int64_t b = 0; b < n_bundles; ++b) {
        std::string tag, text;
        int32_t l = 0, r = 0;
        int64_t np = 0;
        if (!(f >> tag >> l >> r >> np >> text) || tag != "B" || np < 0) { std::fprintf(stderr, "consensus_selftest: bad bundle line\n"); return 2; }
        if (text != "-") bb.insert(bb.end(), text.begin(), text.end());
        bb_off.push_back((int64_t)bb.size()); ovl.push_back(l); ovr.push_back(r);
        for (int64_t p = 0; p < np; ++p) {
            int32_t s = 0, fl = 0;
            int64_t nw = 0;
            if (!(f >> tag >> s >> fl >> nw) || tag != "P" || nw < 0) { std::fprintf(stderr, "consensus_selftest: bad piece line\n"); return 2; }
            for (int64_t i = 0; i < nw; ++i) { uint32_t w = 0; if (!(f >> w)) return 2; cigar.push_back(w); }
            if (!(f >> text)) return 2;
            if (text != "-") bases.insert(bases.end(), text.begin(), text.end());
            sam.push_back(s); flags.push_back(fl); base_off.push_back((int64_t)bases.size()); cig_off.push_back((int64_t)cigar.size());
        }
        piece_off.push_back((int64_t)sam.size());
    }
    hs::ConsensusHost out;
    std::string err;
    if (int rc = hs::consensus_host(n_bundles, bb_off.data(), bb.data(), ovl.data(), ovr.data(), piece_off.data(), sam.data(), flags.data(), base_off.data(), bases.data(),
                                    cig_off.data(), cigar.data(), prm, threads, out, err)) {
        std::fprintf(stderr, "consensus_selftest: %s\n", err.c_str());
        return rc == HS_EINVAL ? 4 : 3;
    }
    for (int64_t b = 0; b < n_bundles; ++b) {
        std::printf("C %lld %d %d %d %d %d %d %d ", (long long)b, out.trim_start[b], out.trim_end[b], out.n_sub[b], out.n_del[b], out.n_ins_bases[b], out.n_low[b], out.n_skipped[b]);
        if (out.cons_off[b + 1] == out.cons_off[b]) std::fputs("-", stdout);
        else std::fwrite(out.cons.data() + out.cons_off[b], 1, (size_t)(out.cons_off[b + 1] - out.cons_off[b]), stdout);
        std::fputc('\n', stdout);
    }
    std::printf("T %lld %lld\n", (long long)out.n_ins_records, (long long)out.n_ins_slots);
    return 0;
}
