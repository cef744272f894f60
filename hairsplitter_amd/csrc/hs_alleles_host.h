// hs_alleles_host.h -- the allele table of include/hairsplitter_hip.h (hs_allele_table): the rule of a cell, stated once for the host
// and the device, and the host side of the table: assembly from what the kernels of hs_kernels_alleles.hip leave, the merge of the
// contig groups' tables, the text of <outfile>.alleles.tsv. No device code and no HIP call in here or in hs_alleles_host.cpp:
// tests/harness/alleles_selftest.cpp builds both into a program of its own.
#ifndef HS_ALLELES_HOST_H
#define HS_ALLELES_HOST_H

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/hairsplitter_hip.h"

#include "hs_rules.h"      // HS_HD

namespace hs {

// What a cell counts over the column entries whose read carries the cell's label (separate_reads.cpp:1056-1113 forms the same per
// intermediate cluster): runs of one pileup code may come in any order, each code once.
struct AlleleCounts {
    uint32_t n = 0, best = 0, second = 0, n_ref = 0, n_alt = 0;
    uint8_t best_code = 0;
    HS_HD void add_run(uint8_t code, uint32_t count, uint8_t ref, uint8_t alt) {
        if (count == 0) return;
        n += count;
        if (code == ref) n_ref += count;
        if (code == alt) n_alt += count;
        if (count > best) { second = best; best = count; best_code = code; }      // best: the largest count; second: the next one, equal to best on a tie
        else {
            if (count == best && code < best_code) best_code = code;               // best_code: the smallest code that has the count best
            if (count > second) second = count;
        }
    }
};
struct AlleleCellValue { uint32_t n, best, second, n_ref, n_alt; uint8_t best_code, call; };
// call = best_code, or 0 (undefined) when secondMax * 2 > max || nb * 0.5 > max (separate_reads.cpp:1100); a tie at the top is always undefined
HS_HD inline AlleleCellValue allele_cell_finish(const AlleleCounts& c) {
    AlleleCellValue v;
    v.n = c.n; v.best = c.best; v.second = c.second; v.n_ref = c.n_ref; v.n_alt = c.n_alt; v.best_code = c.best_code;
    v.call = (c.n == 0 || 2u * c.second > c.best || c.n > 2u * c.best) ? (uint8_t)0 : c.best_code;
    return v;
}


// What one device call leaves, as host arrays: every window and SNP of the call, whether or not it ends up in the table.
struct AlleleRaw {
    int64_t n_windows = 0, n_snps = 0;
    const int32_t* win_contig = nullptr; const int32_t* win_start = nullptr; const int32_t* win_end = nullptr;
    const int32_t* grp_n = nullptr; const int64_t* grp_off = nullptr;      // [n_windows] / [n_windows + 1]: the window's groups lie at grp_ids[grp_off[w] ...]
    const int32_t* grp_ids = nullptr;
    const int32_t* win_snp_first = nullptr; const int32_t* win_snp_last = nullptr;
    const int32_t* snp_contig = nullptr; const int32_t* snp_pos = nullptr; const uint8_t* snp_ref = nullptr; const uint8_t* snp_alt = nullptr;
    const int32_t* snp_win = nullptr;        // -1: the SNP lies in no window
    const int64_t* cell_off = nullptr;       // [n_snps + 1]
    const hs_allele_cell* cells = nullptr; const int32_t* n_calls = nullptr;
    int32_t contig_base = 0;                 // added to every contig index (a contig group of a pipeline)
};
// The table: the windows that have SNPs, in order, their groups, their SNPs, the cells. nullptr and a message in `err` when the raw
// arrays contradict each other (a window whose SNPs are not one range, a column the kernel refused).
hs_allele_table* alleles_assemble(const AlleleRaw& raw, std::string& err);
// the tables of consecutive contig ranges, one after the other (contig order); the parts are left as they are
hs_allele_table* alleles_concat(const std::vector<const hs_allele_table*>& parts);
void alleles_free(hs_allele_table* t);
// <outfile>.alleles.tsv; names[c] = name of contig c (nullptr / too short: the index is printed)
std::string alleles_text(const hs_allele_table* t, const char* const* names, int32_t n_names);
// the three-base context a pileup code stands for (call_variants.cpp:25-31), "." for 0 and for bytes that are no code
std::string allele_context(uint8_t code);
char allele_base(uint8_t code);

}  // namespace hs
#endif
