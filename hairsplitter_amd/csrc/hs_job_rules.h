// hs_job_rules.h -- the reference's rules over a whole JOB (every contig, every read), each stated ONCE for the drivers, the
// pipeline calls, the executables and the test harness (plain C++, host only, no HIP headers). The column rules are in
// hs_rules.h. Every translation unit that includes it is built with -ffp-contract=off. The Python forms are
// dist.mean_of_positive_f32, dist.stage4_error_rate and dist.window_size_from_counts; tests/test_cpu_rules.py holds the two
// sides to each other bit for bit (tests/harness/job_rules_selftest.cpp).
#pragma once
#include <stdint.h>
#include <cstdio>
#include <cstdlib>

namespace hs {

// call_variants.cpp:1312-1315,1377: the float running sum of the positive per-contig mean distances in contig order, divided
// by their count (float / int). No positive entry: 0.0f / 0, a NaN, as the reference prints it.
inline float job_error_rate(const float* mean_distance, int n, int* n_positive) {
    float total = 0; int count = 0;
    for (int c = 0; c < n; ++c) if (mean_distance[c] > 0) { total += mean_distance[c]; count++; }
    if (n_positive) *n_positive = count;
    return total / count;
}

// hairsplitter.py:686-692,725: the text of error_rate.txt read back, capped at 0.15
inline float error_rate_from_text(const char* text) {
    double e = std::strtod(text, nullptr);
    if (e > 0.15) e = 0.15;
    return (float)e;
}

// ... of a value that never went through the file: stage 3 prints it with %g (six significant digits; a NaN stays one)
inline float error_rate_as_stage4_reads_it(float error_rate) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%g", (double)error_rate);
    return error_rate_from_text(buf);
}

// choosing the window size, separate_reads.cpp:1466-1498, over every read of every contig: one read of length `len` counted ...
inline void window_size_count_read(int len, uint32_t& wrapped_sum, int64_t& n_reads, int64_t& above_4000) {
    wrapped_sum += (uint32_t)len;   // `int sumLength` in the reference; wraps the same way
    n_reads++;
    if (len > 4000) above_4000++;
}
// ... and the window size from the counts. No read at all: 0 / 0.0 is a NaN, which fails every comparison: 2000 (where
// the callers of old differed -- a division by zero here, "empty gives mean 4000.0" there -- both ended at 2000 too).
// --amplicon (the longest contig) stays with the callers: they hold different inputs.
inline int32_t window_size_from_counts(uint32_t wrapped_sum, int64_t n_reads, int64_t above_4000) {
    const double mean = (int32_t)wrapped_sum / double(n_reads);
    if (above_4000 < 20 && mean < 4000 && mean > 2000) return 1000;
    if (above_4000 < 20 && mean < 2000) return 500;
    return 2000;
}

}  // namespace hs
