// TEST INFRASTRUCTURE: the device-free half of the split mapper (hs_map_host.h / .cpp: map_reads_split_host, hs_map_segments_text) as a program of its
// own, for tests/test_cpu_map_split.py to hold against the numpy form of tests/map_split_cases.py and for tests/test_gpu_map_split.py to hold the
// device against.
// argv[1]: a text file written by map_split_cases.write_job:
//   k w max_occ band_log2 min_votes extend bucket_bits threads
//   max_segments min_votes min_span max_gap
//   n_contigs, then a line ">" + codes 0..3 per contig; n_reads, then a line per read
// stdout: a line "R <read> n_minimizers n_hits n_skipped read_votes read_second n_segments" per read, a line "S <segment> read contig strand qstart
// qend tstart tend votes second round" per segment, then the PAF lines of hs_map_segments_text. Exit 4: the parameters are refused.
#include "map_job_io.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: map_split_selftest <job.txt>\n"); return 2; }
    std::ifstream f(argv[1]);
    hs_map_params p;
    hs_map_split_params sp;
    int threads = 1;
    if (!read_map_params(f, p, threads) || !(f >> sp.max_segments >> sp.min_votes >> sp.min_span >> sp.max_gap)) {
        std::fprintf(stderr, "map_split_selftest: bad parameter lines\n");
        return 2;
    }
    std::vector<uint8_t> cseq, rseq;
    std::vector<int64_t> coff, roff;
    if (!read_seqs(f, cseq, coff) || !read_seqs(f, rseq, roff)) { std::fprintf(stderr, "map_split_selftest: bad sequences\n"); return 2; }
    const int32_t C = (int32_t)coff.size() - 1, R = (int32_t)roff.size() - 1;
    hs::MapIndexHost ix;
    std::string err;
    if (int rc = hs::map_index_host(cseq.data(), coff.data(), C, p, ix, err)) { std::fprintf(stderr, "map_split_selftest: %s\n", err.c_str()); return rc == HS_EINVAL ? 4 : 3; }
    hs::MapSegmentsHost out;
    if (int rc = hs::map_reads_split_host(ix, sp, rseq.data(), roff.data(), R, threads, out, err)) { std::fprintf(stderr, "map_split_selftest: %s\n", err.c_str()); return rc == HS_EINVAL ? 4 : 3; }
    for (int32_t r = 0; r < R; ++r)
        std::printf("R %d %d %lld %d %d %d %lld\n", r, out.n_minimizers[(size_t)r], (long long)out.n_hits[(size_t)r], out.n_skipped[(size_t)r], out.read_votes[(size_t)r],
                    out.read_second[(size_t)r], (long long)(out.seg_off[(size_t)r + 1] - out.seg_off[(size_t)r]));
    const size_t S = (size_t)out.seg_off[(size_t)R];
    for (size_t s = 0; s < S; ++s)
        std::printf("S %zu %d %d %d %d %d %d %d %d %d %d\n", s, out.read[s], out.contig[s], (int)out.strand[s], out.qstart[s], out.qend[s], out.tstart[s], out.tend[s], out.votes[s],
                    out.second[s], out.round[s]);
    hs_map_segments res{};
    res.n_reads = R; res.n_segments = (int64_t)S; res.seg_off = out.seg_off.data();
    res.read = out.read.data(); res.contig = out.contig.data(); res.strand = out.strand.data(); res.qstart = out.qstart.data(); res.qend = out.qend.data();
    res.tstart = out.tstart.data(); res.tend = out.tend.data(); res.votes = out.votes.data(); res.second = out.second.data(); res.round = out.round.data();
    char* text = nullptr;
    if (hs_map_segments_text(&res, nullptr, roff.data(), nullptr, coff.data(), C, &text)) return 3;
    std::fputs(text, stdout);
    std::free(text);
    return 0;
}
