// hs_haplotypes_host.h -- the text hs_polish_haplotypes_from_files writes (include/hairsplitter_hip.h): one FASTA record per polishing bundle,
// the bundle's consensus without its overhangs. The format is ours: the reference writes no sequence per (contig, interval, group).
// No device code and no HIP call in here: tests/harness/haplotypes_selftest.cpp builds it into a program of its own.
//   header   > contig name _ bundle_start _ bundle_end _ bundle_group      (a group may be -1: the interval that defaults back to the consensus)
//   body     cons[trim_start, trim_end) on one line; an empty line where trim_end <= trim_start
#ifndef HS_HAPLOTYPES_HOST_H
#define HS_HAPLOTYPES_HOST_H

#include <stdint.h>

#include <string>

namespace hs {

// appends the record of one bundle to `out`. cons: the bundle's whole consensus, cons_len bytes; a trim_* outside [0, cons_len] is clamped
inline void haplotype_fasta_record(const std::string& contig, int32_t start, int32_t end, int32_t group, const uint8_t* cons, int64_t cons_len, int32_t trim_start,
                                   int32_t trim_end, std::string& out) {
    out += '>'; out += contig; out += '_'; out += std::to_string(start); out += '_'; out += std::to_string(end); out += '_'; out += std::to_string(group); out += '\n';
    const int64_t n = cons_len < 0 ? 0 : cons_len;
    const int64_t a = trim_start < 0 ? 0 : (trim_start > n ? n : (int64_t)trim_start), e = trim_end > n ? n : (int64_t)trim_end;
    if (cons && e > a) out.append(reinterpret_cast<const char*>(cons) + a, (size_t)(e - a));
    out += '\n';
}

}  // namespace hs

#endif
