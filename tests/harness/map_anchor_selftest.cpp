// TEST INFRASTRUCTURE: the device-free half of the anchored mapper (hs_map_host.h, "anchors" / hs_map_host.cpp: map_anchors_host, map_anchors_of_keys)
// as a program of its own, for tests/test_cpu_map_anchors.py to hold against the numpy form of tests/anchor_cases.py and for
// tests/test_gpu_map_anchors.py to hold the device against.
// argv[1]: a text file written by anchor_cases.write_job, either a job
//   JOB
//   k w max_occ band_log2 min_votes extend bucket_bits threads
//   spacing
//   n_contigs, then a line ">" + codes 0..3 per contig; n_reads, then a line per read
// or the best's hits of one read given as they are
//   HITS
//   spacing Lr n, then n lines "qa t"
// stdout of a job: a line "R <read> " + map_selftest's eleven fields and a line "A <read> n_best n_chain n_supported n_anchors" per read, a line
// "P <read> q t" per anchor. Of hits: "A 0 n n_chain n_supported n_anchors", "C <index into the ordered hits> qa t" per chain member, "P 0 q t" per
// anchor. Exit 4: the parameters are refused.
#include "map_job_io.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: map_anchor_selftest <job.txt>\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string kind;
    f >> kind;
    hs_map_anchor_params ap;
    if (kind == "HITS") {
        long long Lr = 0, n = 0;
        if (!(f >> ap.spacing >> Lr >> n) || n < 0 || n > HS_MAP_ANCHOR_CAPACITY || Lr < 0) { std::fprintf(stderr, "map_anchor_selftest: bad hits header\n"); return 2; }
        if (!hs::map_anchor_params_valid(ap)) return 4;
        std::vector<uint64_t> keys;
        for (long long i = 0; i < n; ++i) {
            int32_t qa, t;
            if (!(f >> qa >> t) || qa < 0 || t < 0) { std::fprintf(stderr, "map_anchor_selftest: bad hit\n"); return 2; }
            keys.push_back(hs::map_anchor_key(qa, t));
        }
        std::vector<int32_t> q, t, members;
        int32_t n_chain = 0, n_supported = 0;
        hs::map_anchors_of_keys(ap, Lr, keys, q, t, &n_chain, &n_supported, &members);
        std::printf("A 0 %lld %d %d %zu\n", n, n_chain, n_supported, q.size());
        for (int32_t m : members) std::printf("C %d %d %d\n", m, hs::map_anchor_qa(keys[(size_t)m]), hs::map_anchor_t(keys[(size_t)m]));
        for (size_t i = 0; i < q.size(); ++i) std::printf("P 0 %d %d\n", q[i], t[i]);
        return 0;
    }
    hs_map_params p;
    int threads = 1;
    if (kind != "JOB" || !read_map_params(f, p, threads) || !(f >> ap.spacing)) {
        std::fprintf(stderr, "map_anchor_selftest: bad parameter lines\n");
        return 2;
    }
    std::vector<uint8_t> cseq, rseq;
    std::vector<int64_t> coff, roff;
    if (!read_seqs(f, cseq, coff) || !read_seqs(f, rseq, roff)) { std::fprintf(stderr, "map_anchor_selftest: bad sequences\n"); return 2; }
    const int32_t C = (int32_t)coff.size() - 1, R = (int32_t)roff.size() - 1;
    hs::MapIndexHost ix;
    std::string err;
    if (int rc = hs::map_index_host(cseq.data(), coff.data(), C, p, ix, err)) { std::fprintf(stderr, "map_anchor_selftest: %s\n", err.c_str()); return rc == HS_EINVAL ? 4 : 3; }
    hs::MapResultHost out;
    hs::MapAnchorsHost an;
    if (int rc = hs::map_anchors_host(ix, ap, rseq.data(), roff.data(), R, threads, out, an, err)) { std::fprintf(stderr, "map_anchor_selftest: %s\n", err.c_str()); return rc == HS_EINVAL ? 4 : 3; }
    for (int32_t r = 0; r < R; ++r) {
        const size_t i = (size_t)r;
        print_read_line(out, r);
        std::printf("A %d %d %d %d %lld\n", r, an.n_best[i], an.n_chain[i], an.n_supported[i], (long long)(an.anc_off[i + 1] - an.anc_off[i]));
        for (int64_t j = an.anc_off[i]; j < an.anc_off[i + 1]; ++j) std::printf("P %d %d %d\n", r, an.anc_q[(size_t)j], an.anc_t[(size_t)j]);
    }
    return 0;
}
