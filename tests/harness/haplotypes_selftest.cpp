// TEST INFRASTRUCTURE: the device-free additions of the haplotype route (hs_haplotypes_host.h: the FASTA record; hs_consensus_host.h: the plan of
// a piece, hs::cons_piece_plan, which k_cons_plan restates on the device) as a program of its own, for tests/test_cpu_haplotypes.py.
// argv[1]: a text file of lines
//   "F <contig> <start> <end> <group> <trim_start> <trim_end> <consensus | ->"      -> the FASTA record of that bundle, as it is written
//   "P <n_bases> <flags> <sam_pos> <L> <n_words> <word> ..."                          -> "PLAN <skipped> <long_cigar> <n_cols> <n_ins>"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "../../hairsplitter_amd/csrc/hs_consensus_host.h"
#include "../../hairsplitter_amd/csrc/hs_haplotypes_host.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: haplotypes_selftest <lines.txt>\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string tag, out;
    while (f >> tag) {
        if (tag == "F") {
            std::string contig, cons;
            int32_t start = 0, end = 0, group = 0, ts = 0, te = 0;
            if (!(f >> contig >> start >> end >> group >> ts >> te >> cons)) { std::fprintf(stderr, "haplotypes_selftest: bad F line\n"); return 2; }
            if (cons == "-") cons.clear();
            hs::haplotype_fasta_record(contig, start, end, group, reinterpret_cast<const uint8_t*>(cons.data()), (int64_t)cons.size(), ts, te, out);
        } else if (tag == "P") {
            int64_t n_bases = 0, sam = 0, L = 0, nw = 0;
            int32_t flags = 0;
            if (!(f >> n_bases >> flags >> sam >> L >> nw) || nw < 0) { std::fprintf(stderr, "haplotypes_selftest: bad P line\n"); return 2; }
            std::vector<uint32_t> w((size_t)nw);
            for (uint32_t& x : w) if (!(f >> x)) return 2;
            const hs::ConsPiecePlan p = hs::cons_piece_plan(w.data(), nw, n_bases, flags, sam, L);
            out += "PLAN " + std::to_string((int)p.skipped) + " " + std::to_string((int)p.long_cigar) + " " + std::to_string(p.n_cols) + " " + std::to_string(p.n_ins) + "\n";
        } else { std::fprintf(stderr, "haplotypes_selftest: unknown line %s\n", tag.c_str()); return 2; }
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
