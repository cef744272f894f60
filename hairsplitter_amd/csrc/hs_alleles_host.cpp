// hs_alleles_host.cpp -- host side of the allele table (hs_alleles_host.h): assembly, merge, text. Plain C++, no device call.
#include "hs_alleles_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace hs {

namespace {
template <class T> T* alloc_n(int64_t n) { return (T*)std::calloc((size_t)(n > 0 ? n : 1), sizeof(T)); }

hs_allele_table* table_alloc(int64_t W, int64_t S, int64_t G, int64_t N) {
    hs_allele_table* t = (hs_allele_table*)std::calloc(1, sizeof(hs_allele_table));
    if (!t) return nullptr;
    t->n_windows = W; t->n_snps = S; t->n_groups = G; t->n_cells = N;
    t->win_contig = alloc_n<int32_t>(W); t->win_start = alloc_n<int32_t>(W); t->win_end = alloc_n<int32_t>(W);
    t->win_group_off = alloc_n<int64_t>(W + 1); t->win_snp_off = alloc_n<int64_t>(W + 1); t->group_ids = alloc_n<int32_t>(G);
    t->snp_contig = alloc_n<int32_t>(S); t->snp_pos = alloc_n<int32_t>(S); t->snp_ref = alloc_n<uint8_t>(S); t->snp_alt = alloc_n<uint8_t>(S);
    t->snp_n_calls = alloc_n<int32_t>(S); t->snp_cell_off = alloc_n<int64_t>(S + 1); t->cells = alloc_n<hs_allele_cell>(N);
    if (!t->win_contig || !t->win_start || !t->win_end || !t->win_group_off || !t->win_snp_off || !t->group_ids || !t->snp_contig || !t->snp_pos ||
        !t->snp_ref || !t->snp_alt || !t->snp_n_calls || !t->snp_cell_off || !t->cells) { alleles_free(t); return nullptr; }
    return t;
}
}  // namespace

void alleles_free(hs_allele_table* t) {
    if (!t) return;
    std::free(t->win_contig); std::free(t->win_start); std::free(t->win_end); std::free(t->win_group_off); std::free(t->win_snp_off); std::free(t->group_ids);
    std::free(t->snp_contig); std::free(t->snp_pos); std::free(t->snp_ref); std::free(t->snp_alt); std::free(t->snp_n_calls); std::free(t->snp_cell_off);
    std::free(t->cells);
    std::free(t);
}

hs_allele_table* alleles_assemble(const AlleleRaw& r, std::string& err) {
    // the windows that have SNPs, and what they hold
    int64_t W = 0, S = 0, G = 0, N = 0;
    int64_t next_snp = 0;      // SNPs ascend with the windows: every window's range begins where the last one ended, SNPs without a window aside
    for (int64_t w = 0; w < r.n_windows; ++w) {
        const int64_t a = r.win_snp_first[w], b = r.win_snp_last[w];
        if (b <= a) continue;
        if (a < next_snp || b > r.n_snps) { err = "allele table: the SNPs of a window are not one ascending range (SNP positions must ascend on every contig)"; return nullptr; }
        for (int64_t s = next_snp; s < a; ++s) if (r.snp_win[s] >= 0) { err = "allele table: a SNP lies outside the range of its window"; return nullptr; }
        for (int64_t s = a; s < b; ++s) {
            if (r.snp_win[s] != w) { err = "allele table: the SNPs of a window are not one ascending range (SNP positions must ascend on every contig)"; return nullptr; }
            if (r.n_calls[s] < 0) { err = "allele table: a column's cells did not fit the cell array"; return nullptr; }
            if (r.cell_off[s + 1] - r.cell_off[s] != r.grp_n[w]) { err = "allele table: cell offsets do not match the groups of the window"; return nullptr; }
        }
        next_snp = b;
        ++W; S += b - a; G += r.grp_n[w]; N += (b - a) * (int64_t)r.grp_n[w];
    }
    for (int64_t s = next_snp; s < r.n_snps; ++s) if (r.snp_win[s] >= 0) { err = "allele table: a SNP lies outside the range of its window"; return nullptr; }
    hs_allele_table* t = table_alloc(W, S, G, N);
    if (!t) { err = "allele table: out of memory"; return nullptr; }
    int64_t wi = 0, si = 0, gi = 0, ni = 0;
    for (int64_t w = 0; w < r.n_windows; ++w) {
        const int64_t a = r.win_snp_first[w], b = r.win_snp_last[w];
        if (b <= a) continue;
        const int32_t g = r.grp_n[w];
        t->win_contig[wi] = r.win_contig[w] + r.contig_base; t->win_start[wi] = r.win_start[w]; t->win_end[wi] = r.win_end[w];
        t->win_group_off[wi] = gi; t->win_snp_off[wi] = si;
        if (g) std::memcpy(t->group_ids + gi, r.grp_ids + r.grp_off[w],(size_t)g * sizeof(int32_t));
        gi += g;
        for (int64_t s = a; s < b; ++s, ++si) {
            t->snp_contig[si] = r.snp_contig[s] + r.contig_base; t->snp_pos[si] = r.snp_pos[s]; t->snp_ref[si] = r.snp_ref[s]; t->snp_alt[si] = r.snp_alt[s];
            t->snp_n_calls[si] = r.n_calls[s]; t->snp_cell_off[si] = ni;
            if (g) std::memcpy(t->cells + ni, r.cells + r.cell_off[s], (size_t)g * sizeof(hs_allele_cell));
            ni += g;
        }
        ++wi;
    }
    t->win_group_off[W] = gi; t->win_snp_off[W] = si; t->snp_cell_off[S] = ni;
    return t;
}

hs_allele_table* alleles_concat(const std::vector<const hs_allele_table*>& parts) {
    int64_t W = 0, S = 0, G = 0, N = 0;
    for (const hs_allele_table* p : parts) if (p) { W += p->n_windows; S += p->n_snps; G += p->n_groups; N += p->n_cells; }
    hs_allele_table* t = table_alloc(W, S, G, N);
    if (!t) return nullptr;
    int64_t w0 = 0, s0 = 0, g0 = 0, n0 = 0;
    for (const hs_allele_table* p : parts) {
        if (!p) continue;
        auto cp = [](void* d, const void* s, size_t n) { if (n) std::memcpy(d, s, n); };
        cp(t->win_contig + w0, p->win_contig, (size_t)p->n_windows * 4); cp(t->win_start + w0, p->win_start, (size_t)p->n_windows * 4);
        cp(t->win_end + w0, p->win_end, (size_t)p->n_windows * 4); cp(t->group_ids + g0, p->group_ids, (size_t)p->n_groups * 4);
        cp(t->snp_contig + s0, p->snp_contig, (size_t)p->n_snps * 4); cp(t->snp_pos + s0, p->snp_pos, (size_t)p->n_snps * 4);
        cp(t->snp_ref + s0, p->snp_ref, (size_t)p->n_snps); cp(t->snp_alt + s0, p->snp_alt, (size_t)p->n_snps);
        cp(t->snp_n_calls + s0, p->snp_n_calls, (size_t)p->n_snps * 4); cp(t->cells + n0, p->cells, (size_t)p->n_cells * sizeof(hs_allele_cell));
        for (int64_t w = 0; w < p->n_windows; ++w) { t->win_group_off[w0 + w] = g0 + p->win_group_off[w]; t->win_snp_off[w0 + w] = s0 + p->win_snp_off[w]; }
        for (int64_t s = 0; s < p->n_snps; ++s) t->snp_cell_off[s0 + s] = n0 + p->snp_cell_off[s];
        t->t_kernel_ms += p->t_kernel_ms; t->n_entries += p->n_entries; t->n_wide_columns += p->n_wide_columns;
        w0 += p->n_windows; s0 += p->n_snps; g0 += p->n_groups; n0 += p->n_cells;
    }
    t->win_group_off[W] = g0; t->win_snp_off[W] = s0; t->snp_cell_off[S] = n0;
    return t;
}

char allele_base(uint8_t code) { return (code >= 33 && code < 33 + 125) ? "ACGT-"[(code - 33) % 5] : '.'; }
std::string allele_context(uint8_t code) {
    if (code < 33 || code >= 33 + 125) return ".";
    const int v = code - 33;
    const char s[4] = {"ACGT-"[(v % 25) / 5], "ACGT-"[v % 5], "ACGT-"[v / 25], 0};
    return s;
}

std::string alleles_text(const hs_allele_table* t, const char* const* names, int32_t n_names) {
    std::string out;
    if (!t) return out;
    char buf[96];
    for (int64_t w = 0; w < t->n_windows; ++w) {
        const int32_t c = t->win_contig[w];
        out += "WINDOW\t";
        if (names && c >= 0 && c < n_names && names[c]) out += names[c]; else { std::snprintf(buf, sizeof buf, "%d", c); out += buf; }
        std::snprintf(buf, sizeof buf, "\t%d\t%d\t", t->win_start[w], t->win_end[w]); out += buf;
        const int64_t g0 = t->win_group_off[w], g1 = t->win_group_off[w + 1];
        for (int64_t g = g0; g < g1; ++g) { std::snprintf(buf, sizeof buf, "%d,", t->group_ids[g]); out += buf; }
        out += '\n';
        for (int64_t s = t->win_snp_off[w]; s < t->win_snp_off[w + 1]; ++s) {
            std::snprintf(buf, sizeof buf, "SNP\t%d\t%c\t%c\t%d", t->snp_pos[s], allele_base(t->snp_ref[s]), allele_base(t->snp_alt[s]), t->snp_n_calls[s]); out += buf;
            const hs_allele_cell* cell = t->cells + t->snp_cell_off[s];
            for (int64_t g = g0; g < g1; ++g) {
                const hs_allele_cell& x = cell[g - g0];
                std::snprintf(buf, sizeof buf, "\t%d:%u:%u:%u:", t->group_ids[g], (unsigned)x.n, (unsigned)x.n_ref, (unsigned)x.n_alt); out += buf;
                out += allele_context(x.call);
            }
            out += '\n';
        }
    }
    return out;
}

}  // namespace hs

extern "C" {
void hs_allele_table_destroy(hs_allele_table* t) { hs::alleles_free(t); }
int hs_alleles_text(const hs_allele_table* t, const char* const* names, int32_t n_names, char** out) {
    if (!t || !out) return HS_EINVAL;
    const std::string s = hs::alleles_text(t, names, n_names);
    *out = (char*)std::malloc(s.size() + 1);
    if (!*out) return HS_EINVAL;
    std::memcpy(*out, s.c_str(), s.size() + 1);
    return HS_OK;
}
}
