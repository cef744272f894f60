// TEST INFRASTRUCTURE: the host side of the allele table (hs_alleles_host.h / .cpp -- the cell rule the kernel ends in, the assembly of the
// table from what the kernels leave, the merge of the contig groups' tables, the text of <outfile>.alleles.tsv) without a device, for
// tests/test_cpu_alleles_host.py to hold against tests/allele_cases.py. The arrays the kernels would leave (window of every SNP, group
// lists, SNP ranges, cell offsets, cells) are formed here by a plain walk that ends in the same hs::AlleleCounts / allele_cell_finish.
// stdin: "<C> <split>", per contig "<n_reads> <n_snps>" and per SNP "<pos> <ref> <alt> <depth>" + depth pairs "<read> <code>", then
// "<W>", win_off [C + 1], per window "<start> <end>" + one label per read of its contig. The contigs [0, split) and [split, C) are
// assembled as two parts (a pipeline's contig groups) and merged. stdout: the text, contigs named c0, c1, ...
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "../../hairsplitter_amd/csrc/hs_alleles_host.h"

struct Contig { int n_reads = 0; std::vector<int32_t> pos; std::vector<uint8_t> ref, alt; std::vector<int64_t> off{0}; std::vector<int32_t> idx; std::vector<uint8_t> code; };

static hs_allele_table* part(const std::vector<Contig>& cs, const std::vector<int64_t>& win_off, const std::vector<int32_t>& ws, const std::vector<int32_t>& we,
                             const std::vector<std::vector<int32_t>>& labels, int c0, int c1) {
    std::vector<int32_t> win_contig, win_start, win_end, grp_n, grp_ids, first, last, snp_contig, snp_pos, snp_win, n_calls;
    std::vector<uint8_t> snp_ref, snp_alt;
    std::vector<int64_t> grp_off(1, 0), cell_off(1, 0);
    std::vector<hs_allele_cell> cells;
    const int64_t w_base = win_off[(size_t)c0];
    for (int c = c0; c < c1; ++c)
        for (int64_t w = win_off[(size_t)c]; w < win_off[(size_t)c + 1]; ++w) { win_contig.push_back(c - c0); win_start.push_back(ws[(size_t)w]); win_end.push_back(we[(size_t)w]); }
    const size_t W = win_start.size();
    grp_n.assign(W, 0); first.assign(W, 0); last.assign(W, 0);
    std::vector<std::vector<int32_t>> groups(W);
    // window of every SNP, then the groups of the windows that have some
    for (int c = c0; c < c1; ++c)
        for (size_t s = 0; s < cs[(size_t)c].pos.size(); ++s) {
            int32_t win = -1;
            for (int64_t w = win_off[(size_t)c]; w < win_off[(size_t)c + 1] && win < 0; ++w)
                if (ws[(size_t)w] <= cs[(size_t)c].pos[s] && cs[(size_t)c].pos[s] <= we[(size_t)w]) win = (int32_t)(w - w_base);
            const int32_t k = (int32_t)snp_pos.size();
            if (win >= 0) { if (snp_win.empty() || snp_win.back() != win) first[(size_t)win] = k; last[(size_t)win] = k + 1; }
            snp_contig.push_back(c - c0); snp_pos.push_back(cs[(size_t)c].pos[s]); snp_ref.push_back(cs[(size_t)c].ref[s]); snp_alt.push_back(cs[(size_t)c].alt[s]);
            snp_win.push_back(win);
        }
    for (size_t w = 0; w < W; ++w) {
        if (last[w] > first[w]) {
            for (int32_t l : labels[(size_t)w_base + w]) if (l >= 0) groups[w].push_back(l);
            std::sort(groups[w].begin(), groups[w].end());
            groups[w].erase(std::unique(groups[w].begin(), groups[w].end()), groups[w].end());
        }
        grp_n[w] = (int32_t)groups[w].size();
        grp_ids.insert(grp_ids.end(), groups[w].begin(), groups[w].end());
        grp_off.push_back((int64_t)grp_ids.size());
    }
    // the cells
    {
        size_t k = 0;
        for (int c = c0; c < c1; ++c)
            for (size_t s = 0; s < cs[(size_t)c].pos.size(); ++s, ++k) {
                const Contig& ct = cs[(size_t)c];
                const int32_t win = snp_win[k];
                int32_t calls = 0;
                if (win >= 0) {
                    const std::vector<int32_t>& lab = labels[(size_t)w_base + (size_t)win];
                    bool seen[256] = {false};
                    for (int32_t g : groups[(size_t)win]) {
                        std::map<uint8_t, uint32_t> runs;
                        for (int64_t e = ct.off[s]; e < ct.off[s + 1]; ++e)
                            if (ct.idx[(size_t)e] >= 0 && ct.idx[(size_t)e] < (int32_t)lab.size() && lab[(size_t)ct.idx[(size_t)e]] == g) runs[ct.code[(size_t)e]]++;
                        hs::AlleleCounts acc;
                        for (const auto& r : runs) acc.add_run(r.first, r.second, ct.ref[s], ct.alt[s]);
                        const hs::AlleleCellValue v = hs::allele_cell_finish(acc);
                        hs_allele_cell x;
                        x.n = (uint16_t)v.n; x.best = (uint16_t)v.best; x.second = (uint16_t)v.second; x.n_ref = (uint16_t)v.n_ref; x.n_alt = (uint16_t)v.n_alt;
                        x.best_code = v.best_code; x.call = v.call;
                        cells.push_back(x);
                        if (v.call && !seen[v.call]) { seen[v.call] = true; ++calls; }
                    }
                }
                n_calls.push_back(calls);
                cell_off.push_back((int64_t)cells.size());
            }
    }
    hs::AlleleRaw raw;
    raw.n_windows = (int64_t)W; raw.n_snps = (int64_t)snp_pos.size();
    raw.win_contig = win_contig.data(); raw.win_start = win_start.data(); raw.win_end = win_end.data();
    raw.grp_n = grp_n.data(); raw.grp_off = grp_off.data(); raw.grp_ids = grp_ids.data(); raw.win_snp_first = first.data(); raw.win_snp_last = last.data();
    raw.snp_contig = snp_contig.data(); raw.snp_pos = snp_pos.data(); raw.snp_ref = snp_ref.data(); raw.snp_alt = snp_alt.data(); raw.snp_win = snp_win.data();
    raw.cell_off = cell_off.data(); raw.cells = cells.data(); raw.n_calls = n_calls.data(); raw.contig_base = c0;
    std::string err;
    hs_allele_table* t = hs::alleles_assemble(raw, err);
    if (!t) std::fprintf(stderr, "alleles_selftest: %s\n", err.c_str());
    return t;
}

int main() {
    int C = 0, split = 0;
    if (std::scanf("%d %d", &C, &split) != 2 || C < 0 || split < 0 || split > C) return 2;
    std::vector<Contig> cs((size_t)C);
    for (Contig& c : cs) {
        int n_snps = 0;
        if (std::scanf("%d %d", &c.n_reads, &n_snps) != 2) return 2;
        for (int s = 0; s < n_snps; ++s) {
            int pos, ref, alt, depth;
            if (std::scanf("%d %d %d %d", &pos, &ref, &alt, &depth) != 4) return 2;
            c.pos.push_back(pos); c.ref.push_back((uint8_t)ref); c.alt.push_back((uint8_t)alt);
            for (int e = 0; e < depth; ++e) { int r, k; if (std::scanf("%d %d", &r, &k) != 2) return 2; c.idx.push_back(r); c.code.push_back((uint8_t)k); }
            c.off.push_back((int64_t)c.idx.size());
        }
    }
    int W = 0;
    if (std::scanf("%d", &W) != 1 || W < 0) return 2;
    std::vector<int64_t> win_off((size_t)C + 1);
    for (int64_t& v : win_off) { long long x; if (std::scanf("%lld", &x) != 1) return 2; v = x; }
    std::vector<int32_t> ws((size_t)W), we((size_t)W);
    std::vector<std::vector<int32_t>> labels((size_t)W);
    for (int c = 0; c < C; ++c)
        for (int64_t w = win_off[(size_t)c]; w < win_off[(size_t)c + 1]; ++w) {
            if (w < 0 || w >= W || std::scanf("%d %d", &ws[(size_t)w], &we[(size_t)w]) != 2) return 2;
            labels[(size_t)w].resize((size_t)cs[(size_t)c].n_reads);
            for (int32_t& l : labels[(size_t)w]) if (std::scanf("%d", &l) != 1) return 2;
        }
    hs_allele_table* a = part(cs, win_off, ws, we, labels, 0, split);
    hs_allele_table* b = part(cs, win_off, ws, we, labels, split, C);
    if (!a || !b) return 3;
    hs_allele_table* t = hs::alleles_concat({a, b});
    if (!t) return 3;
    std::vector<std::string> names;
    for (int c = 0; c < C; ++c) names.push_back("c" + std::to_string(c));
    std::vector<const char*> np;
    for (const std::string& s : names) np.push_back(s.c_str());
    char* text = nullptr;
    if (hs_alleles_text(t, np.data(), (int32_t)np.size(), &text)) return 3;
    std::fputs(text, stdout);
    std::free(text);
    hs_allele_table_destroy(a); hs_allele_table_destroy(b); hs_allele_table_destroy(t);
    return 0;
}
