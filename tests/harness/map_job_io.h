// TEST INFRASTRUCTURE: what the three mapper selftests (map_selftest, map_split_selftest, map_anchor_selftest) read and print alike -- the
// hs_map_params line of a job file, its sequences, and the "R" line of a read's eleven fields.
#ifndef HS_TESTS_MAP_JOB_IO_H
#define HS_TESTS_MAP_JOB_IO_H
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "../../hairsplitter_amd/csrc/hs_map_host.h"

// "k w max_occ band_log2 min_votes extend bucket_bits threads"
inline bool read_map_params(std::ifstream& f, hs_map_params& p, int& threads) {
    return (bool)(f >> p.k >> p.w >> p.max_occ >> p.band_log2 >> p.min_votes >> p.extend >> p.bucket_bits >> threads);
}

// a count, then a line ">" + codes 0..3 per sequence
inline bool read_seqs(std::ifstream& f, std::vector<uint8_t>& seq, std::vector<int64_t>& off) {
    long n = -1;
    std::string line;
    if (!(f >> n) || n < 0) return false;
    std::getline(f, line);
    off.assign(1, 0);
    for (long i = 0; i < n; ++i) {
        if (!std::getline(f, line) || line.empty() || line[0] != '>') return false;
        for (size_t c = 1; c < line.size(); ++c) {
            if (line[c] < '0' || line[c] > '3') return false;
            seq.push_back((uint8_t)(line[c] - '0'));
        }
        off.push_back((int64_t)seq.size());
    }
    return true;
}

// "R <read> contig strand qstart qend tstart tend votes second n_minimizers n_hits n_skipped"
inline void print_read_line(const hs::MapResultHost& out, int32_t r) {
    const size_t i = (size_t)r;
    std::printf("R %d %d %d %d %d %d %d %d %d %d %lld %d\n", r, out.contig[i], (int)out.strand[i], out.qstart[i], out.qend[i], out.tstart[i], out.tend[i], out.votes[i], out.second[i],
                out.n_minimizers[i], (long long)out.n_hits[i], out.n_skipped[i]);
}
#endif
