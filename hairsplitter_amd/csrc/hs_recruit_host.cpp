// hs_recruit_host.cpp -- host side of the recruit table (hs_recruit_host.h): assembly, merge, apply, text. Plain C++, no device call.
#include "hs_recruit_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace hs {

namespace {
template <class T> T* alloc_n(int64_t n) { return (T*)std::calloc((size_t)(n > 0 ? n : 1), sizeof(T)); }

hs_recruit_table* table_alloc(int64_t W, int64_t R) {
    hs_recruit_table* t = (hs_recruit_table*)std::calloc(1, sizeof(hs_recruit_table));
    if (!t) return nullptr;
    t->n_windows = W; t->n_rows = R;
    t->win_contig = alloc_n<int32_t>(W); t->win_start = alloc_n<int32_t>(W); t->win_end = alloc_n<int32_t>(W);
    t->win_index = alloc_n<int64_t>(W); t->win_row_off = alloc_n<int64_t>(W + 1); t->rows = alloc_n<hs_recruit_row>(R);
    if (!t->win_contig || !t->win_start || !t->win_end || !t->win_index || !t->win_row_off || !t->rows) { recruit_free(t); return nullptr; }
    return t;
}
}  // namespace

void recruit_free(hs_recruit_table* t) {
    if (!t) return;
    std::free(t->win_contig); std::free(t->win_start); std::free(t->win_end); std::free(t->win_index); std::free(t->win_row_off); std::free(t->rows);
    std::free(t);
}

hs_recruit_table* recruit_assemble(const RecruitRaw& r, std::string& err) {
    int64_t W = 0, R = 0;
    for (int64_t w = 0; w < r.n_windows; ++w) {
        const int64_t n = r.win_row_off[w + 1] - r.win_row_off[w];
        const bool has_snp = r.win_snp_last[w] > r.win_snp_first[w];
        if (n < 0 || (!has_snp && n != 0)) { err = "recruit table: a window without SNPs has rows, or row offsets descend"; return nullptr; }
        if (has_snp) { ++W; R += n; }
    }
    if (r.n_windows > 0 && (r.win_row_off[0] != 0 || r.win_row_off[r.n_windows] != R)) { err = "recruit table: row offsets do not cover the rows"; return nullptr; }
    hs_recruit_table* t = table_alloc(W, R);
    if (!t) { err = "recruit table: out of memory"; return nullptr; }
    int64_t wi = 0;
    for (int64_t w = 0; w < r.n_windows; ++w) {
        if (r.win_snp_last[w] <= r.win_snp_first[w]) continue;
        t->win_contig[wi] = r.win_contig[w] + r.contig_base; t->win_start[wi] = r.win_start[w]; t->win_end[wi] = r.win_end[w];
        t->win_index[wi] = w; t->win_row_off[wi] = r.win_row_off[w];
        ++wi;
    }
    t->win_row_off[W] = R;
    if (R) std::memcpy(t->rows, r.rows, (size_t)R * sizeof(hs_recruit_row));
    for (int64_t i = 0; i < R; ++i) t->n_assigned += t->rows[i].assigned != 0;
    t->params = r.params; t->n_call_windows = r.n_windows;
    return t;
}

hs_recruit_table* recruit_concat(const std::vector<const hs_recruit_table*>& parts) {
    int64_t W = 0, R = 0;
    for (const hs_recruit_table* p : parts) if (p) { W += p->n_windows; R += p->n_rows; }
    hs_recruit_table* t = table_alloc(W, R);
    if (!t) return nullptr;
    int64_t w0 = 0, r0 = 0, call_w0 = 0;
    bool first = true;
    for (const hs_recruit_table* p : parts) {
        if (!p) continue;
        auto cp = [](void* d, const void* s, size_t n) { if (n) std::memcpy(d, s, n); };
        cp(t->win_contig + w0, p->win_contig, (size_t)p->n_windows * 4); cp(t->win_start + w0, p->win_start, (size_t)p->n_windows * 4);
        cp(t->win_end + w0, p->win_end, (size_t)p->n_windows * 4); cp(t->rows + r0, p->rows, (size_t)p->n_rows * sizeof(hs_recruit_row));
        for (int64_t w = 0; w < p->n_windows; ++w) { t->win_index[w0 + w] = call_w0 + p->win_index[w]; t->win_row_off[w0 + w] = r0 + p->win_row_off[w]; }
        if (first) { t->params = p->params; first = false; }
        t->n_assigned += p->n_assigned; t->n_counter_words += p->n_counter_words; t->n_entries += p->n_entries; t->t_kernel_ms += p->t_kernel_ms;
        w0 += p->n_windows; r0 += p->n_rows; call_w0 += p->n_call_windows;
    }
    t->win_row_off[W] = r0; t->n_call_windows = call_w0;
    return t;
}

std::string recruit_text(const hs_recruit_table* t, const char* const* names, int32_t n_names) {
    std::string out;
    if (!t) return out;
    char buf[192];
    for (int64_t w = 0; w < t->n_windows; ++w) {
        const int32_t c = t->win_contig[w];
        out += "WINDOW\t";
        if (names && c >= 0 && c < n_names && names[c]) out += names[c]; else { std::snprintf(buf, sizeof buf, "%d", c); out += buf; }
        std::snprintf(buf, sizeof buf, "\t%d\t%d\n", t->win_start[w], t->win_end[w]); out += buf;
        for (int64_t i = t->win_row_off[w]; i < t->win_row_off[w + 1]; ++i) {
            const hs_recruit_row& r = t->rows[i];
            std::snprintf(buf, sizeof buf, "READ\t%d\t%d\t%d\t%u\t%u\t%d\t%u\t%u\t%u\t%d\n", r.read, r.label, r.best_group, r.m_best, r.x_best, r.second_group,
                          r.m_second, r.x_second, r.n_entries, r.assigned ? 1 : 0);
            out += buf;
        }
    }
    return out;
}

}  // namespace hs

extern "C" {
hs_recruit_params hs_recruit_params_default(void) {
    hs_recruit_params p;
    p.which = HS_RECRUIT_ABSENT | HS_RECRUIT_UNCLUSTERED; p.min_informative = 3; p.min_margin = 2; p.mismatch_num = 1; p.mismatch_den = 4;
    return p;
}
void hs_recruit_table_destroy(hs_recruit_table* t) { hs::recruit_free(t); }
int hs_recruit_apply(const hs_recruit_table* t, const int64_t* label_off, const int32_t* labels_in, int32_t* labels_out, int64_t n_labels) {
    if (!t || n_labels < 0 || (n_labels > 0 && (!labels_in || !labels_out)) || (t->n_rows > 0 && !label_off)) return HS_EINVAL;
    if (n_labels > 0 && labels_out != labels_in) std::memmove(labels_out, labels_in, (size_t)n_labels * sizeof(int32_t));
    for (int64_t w = 0; w < t->n_windows; ++w) {
        if (t->win_row_off[w + 1] == t->win_row_off[w]) continue;
        const int64_t wi = t->win_index[w];
        if (wi < 0 || wi >= t->n_call_windows) return HS_EINVAL;
        const int64_t l0 = label_off[wi], l1 = label_off[wi + 1];
        if (l0 < 0 || l1 < l0 || l1 > n_labels) return HS_EINVAL;
        for (int64_t i = t->win_row_off[w]; i < t->win_row_off[w + 1]; ++i) {
            const hs_recruit_row& r = t->rows[i];
            if (r.read < 0 || r.read >= l1 - l0) return HS_EINVAL;
            if (r.assigned && r.best_group >= 0 && labels_out[l0 + r.read] < 0) labels_out[l0 + r.read] = r.best_group;
        }
    }
    return HS_OK;
}
int hs_recruit_text(const hs_recruit_table* t, const char* const* names, int32_t n_names, char** out) {
    if (!t || !out) return HS_EINVAL;
    const std::string s = hs::recruit_text(t, names, n_names);
    *out = (char*)std::malloc(s.size() + 1);
    if (!*out) return HS_EINVAL;
    std::memcpy(*out, s.c_str(), s.size() + 1);
    return HS_OK;
}
}
