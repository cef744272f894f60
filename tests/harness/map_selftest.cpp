// TEST INFRASTRUCTURE: the device-free half of the read mapper (hs_map_host.h / .cpp -- the rule functions the kernels end in, and the whole job on
// the host) as a program of its own, for tests/test_cpu_map_cases.py to hold against the numpy form of tests/map_cases.py and for
// tests/test_gpu_map.py to hold the device against.
// argv[1]: a text file written by map_cases.write_job:
//   k w max_occ band_log2 min_votes extend bucket_bits threads
//   n_contigs, then a line ">" + codes 0..3 per contig; n_reads, then a line per read
// stdout: "INDEX <bucket_bits> <n_entries>", a line "E <bucket> <hash> <contig> <t> <strand bit>" per entry (bucket, hash, contig, t ascending),
// a line "M <read> <q> <strand bit> <hash>" per read minimizer, a line "R <read> contig strand qstart qend tstart tend votes second n_minimizers
// n_hits n_skipped" per read, then the PAF lines of hs_map_text. Exit 4: the parameters are refused.
#include "map_job_io.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: map_selftest <job.txt>\n"); return 2; }
    std::ifstream f(argv[1]);
    hs_map_params p;
    int threads = 1;
    if (!read_map_params(f, p, threads)) { std::fprintf(stderr, "map_selftest: bad parameter line\n"); return 2; }
    std::vector<uint8_t> cseq, rseq;
    std::vector<int64_t> coff, roff;
    if (!read_seqs(f, cseq, coff) || !read_seqs(f, rseq, roff)) { std::fprintf(stderr, "map_selftest: bad sequences\n"); return 2; }
    const int32_t C = (int32_t)coff.size() - 1, R = (int32_t)roff.size() - 1;
    hs::MapIndexHost ix;
    std::string err;
    if (int rc = hs::map_index_host(cseq.data(), coff.data(), C, p, ix, err)) { std::fprintf(stderr, "map_selftest: %s\n", err.c_str()); return rc == HS_EINVAL ? 4 : 3; }
    std::printf("INDEX %d %zu\n", ix.bucket_bits, ix.e_h.size());
    for (size_t b = 0; b + 1 < ix.bucket_off.size(); ++b)
        for (int64_t e = ix.bucket_off[b]; e < ix.bucket_off[b + 1]; ++e)
            std::printf("E %zu %u %d %u %u\n", b, ix.e_h[(size_t)e], ix.e_c[(size_t)e], ix.e_ts[(size_t)e] >> 1, ix.e_ts[(size_t)e] & 1u);
    hs::MapMinimizers mz;
    hs::map_minimizers(rseq.data(), roff.data(), R, p, mz);
    for (size_t i = 0; i < mz.h.size(); ++i) std::printf("M %d %u %u %u\n", mz.seq[i], mz.ps[i] >> 1, mz.ps[i] & 1u, mz.h[i]);
    hs::MapResultHost out;
    if (hs::map_reads_host(ix, rseq.data(), roff.data(), R, threads, out, err)) { std::fprintf(stderr, "map_selftest: %s\n", err.c_str()); return 3; }
    for (int32_t r = 0; r < R; ++r) print_read_line(out, r);
    hs_map_result res{};
    res.n_reads = R;
    res.contig = out.contig.data(); res.strand = out.strand.data(); res.qstart = out.qstart.data(); res.qend = out.qend.data(); res.tstart = out.tstart.data();
    res.tend = out.tend.data(); res.votes = out.votes.data(); res.second = out.second.data();
    char* text = nullptr;
    if (hs_map_text(&res, nullptr, roff.data(), nullptr, coff.data(), C, &text)) return 3;
    std::fputs(text, stdout);
    std::free(text);
    return 0;
}
