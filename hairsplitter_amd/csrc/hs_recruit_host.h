// hs_recruit_host.h -- the recruit table of include/hairsplitter_hip.h (hs_recruit_table): the rule that crosses a window's unlabelled reads
// with the allele calls of its groups, stated once for the host and the device, and the host side of the table: assembly from what the
// kernels of hs_kernels_recruit.hip leave, the merge of the contig groups' tables, hs_recruit_apply, the text of <outfile>.recruit.tsv.
// No device code and no HIP call in here or in hs_recruit_host.cpp: tests/harness/recruit_selftest.cpp builds both into a program of its own.
#ifndef HS_RECRUIT_HOST_H
#define HS_RECRUIT_HOST_H

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/hairsplitter_hip.h"

#include "hs_rules.h"      // HS_HD

namespace hs {

// thresholds the call accepts (anything else: HS_EINVAL)
HS_HD inline bool recruit_params_valid(const hs_recruit_params& p) {
    return p.min_informative >= 1 && p.min_margin >= 1 && p.mismatch_den >= 1 && p.mismatch_num >= 0 && p.mismatch_num <= p.mismatch_den;
}
// is a read with this label in a window a row of the table?
HS_HD inline bool recruit_selected(int32_t label, int32_t which) {
    return label >= 0 ? (which & HS_RECRUIT_LABELLED) != 0 : label == -1 ? (which & HS_RECRUIT_UNCLUSTERED) != 0 : label == -2 ? (which & HS_RECRUIT_ABSENT) != 0 : false;
}
// one column entry against the call of one group's cell: 0 not counted (the call is undefined), 1 a match, 2 a mismatch. Any code can match.
HS_HD inline int recruit_entry(uint8_t code, uint8_t call) { return call == 0 ? 0 : (code == call ? 1 : 2); }

// best and second group of a row: candidates (group slot k, m_k, x_k) offered in any order, each once. One candidate beats another by the larger
// score m - x (signed), then by the smaller slot -- slots ascend with the ids.
struct RecruitChoice {
    int32_t best = -1, second = -1;
    uint32_t m_best = 0, x_best = 0, m_second = 0, x_second = 0;
    HS_HD static bool beats(int32_t ka, uint32_t ma, uint32_t xa, int32_t kb, uint32_t mb, uint32_t xb) {
        const int64_t sa = (int64_t)ma - (int64_t)xa, sb = (int64_t)mb - (int64_t)xb;
        return sa > sb || (sa == sb && ka < kb);
    }
    HS_HD void offer(int32_t k, uint32_t m, uint32_t x) {
        if (k < 0) return;
        if (best < 0 || beats(k, m, x, best, m_best, x_best)) {
            second = best; m_second = m_best; x_second = x_best;
            best = k; m_best = m; x_best = x;
        } else if (second < 0 || beats(k, m, x, second, m_second, x_second)) {
            second = k; m_second = m; x_second = x;
        }
    }
    HS_HD void merge(const RecruitChoice& o) { offer(o.best, o.m_best, o.x_best); offer(o.second, o.m_second, o.x_second); }      // (disjoint candidates)
};
// (a) enough informative entries, (b) the margin over the second group (vacuous with one group), (c) the mismatch share, in 64 bits
HS_HD inline int32_t recruit_assigned(const hs_recruit_params& p, int32_t n_groups, const RecruitChoice& c) {
    if (c.best < 0) return 0;
    const int64_t inf = (int64_t)c.m_best + (int64_t)c.x_best;
    if (inf < (int64_t)p.min_informative) return 0;
    if (n_groups != 1) {
        const int64_t sb = (int64_t)c.m_best - (int64_t)c.x_best, ss = (int64_t)c.m_second - (int64_t)c.x_second;
        if (c.second < 0 || sb - ss < (int64_t)p.min_margin) return 0;
    }
    return (int64_t)c.x_best * (int64_t)p.mismatch_den <= (int64_t)p.mismatch_num * inf ? 1 : 0;
}
// the row record of a choice; ids = the window's group ids by slot
HS_HD inline hs_recruit_row recruit_row(const hs_recruit_params& p, int32_t read, int32_t label, int32_t n_groups, const int32_t* ids, const RecruitChoice& c, uint32_t n_entries) {
    hs_recruit_row r;
    r.read = read; r.label = label;
    r.best_group = c.best >= 0 ? ids[c.best] : -1; r.second_group = c.second >= 0 ? ids[c.second] : -1;
    r.m_best = c.m_best; r.x_best = c.x_best; r.m_second = c.second >= 0 ? c.m_second : 0; r.x_second = c.second >= 0 ? c.x_second : 0;
    r.n_entries = n_entries; r.assigned = recruit_assigned(p, n_groups, c);
    return r;
}

// What one device call leaves, as host arrays: every window of the call, whether or not it ends up in the table (the table holds the windows
// that have SNPs, as the allele table does).
struct RecruitRaw {
    int64_t n_windows = 0;
    const int32_t* win_contig = nullptr; const int32_t* win_start = nullptr; const int32_t* win_end = nullptr;
    const int32_t* win_snp_first = nullptr; const int32_t* win_snp_last = nullptr;      // the allele plan's: first < last = the window has SNPs
    const int64_t* win_row_off = nullptr;      // [n_windows + 1] rows of window w = rows[win_row_off[w] ...], read ascending
    const hs_recruit_row* rows = nullptr;
    int32_t contig_base = 0;
    hs_recruit_params params{};
};
hs_recruit_table* recruit_assemble(const RecruitRaw& raw, std::string& err);
// the tables of consecutive contig ranges, one after the other (contig order); the parts are left as they are
hs_recruit_table* recruit_concat(const std::vector<const hs_recruit_table*>& parts);
void recruit_free(hs_recruit_table* t);
// <outfile>.recruit.tsv; names[c] = name of contig c (nullptr / too short: the index is printed)
std::string recruit_text(const hs_recruit_table* t, const char* const* names, int32_t n_names);

}  // namespace hs
#endif
