// TEST INFRASTRUCTURE: the host side of the recruit table (hs_recruit_host.h / .cpp -- the rule functions the kernels end in, the assembly of the
// table from what the kernels leave, the merge of the contig groups' tables, hs_recruit_apply, the text of <outfile>.recruit.tsv) without a
// device, for tests/test_cpu_recruit_host.py to hold against tests/recruit_cases.py. What the kernels would be given (columns, dense labels,
// the allele plan and the calls of its cells) comes as JSON, one object of integer arrays written by recruit_cases.host_input; the flags,
// counters and rows are formed here by a plain walk that ends in the same hs::recruit_selected / recruit_entry / RecruitChoice / recruit_row.
// argv[1]: the JSON file. The contigs [0, split) and [split, C) are assembled as two parts (a pipeline's contig groups) and merged.
// stdout: the text (contigs named c0, c1, ...), a line "LABELS" and the labels after hs_recruit_apply, one line. Exit 4: the parameters are refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../../hairsplitter_amd/csrc/hs_recruit_host.h"

typedef std::vector<long long> Arr;

static bool parse(const std::string& s, std::map<std::string, Arr>& out) {      // {"key": [1, 2, ...], ...}
    size_t i = 0;
    while ((i = s.find('"', i)) != std::string::npos) {
        const size_t e = s.find('"', i + 1);
        if (e == std::string::npos) return false;
        const std::string key = s.substr(i + 1, e - i - 1);
        size_t a = s.find('[', e);
        const size_t b = a == std::string::npos ? a : s.find(']', a);
        if (b == std::string::npos) return false;
        Arr& v = out[key];
        const char* p = s.c_str() + a + 1;
        const char* end = s.c_str() + b;
        while (p < end) {
            char* q = nullptr;
            const long long x = std::strtoll(p, &q, 10);
            if (q == p) { ++p; continue; }
            v.push_back(x); p = q;
        }
        i = b + 1;
    }
    return true;
}

struct Call {
    Arr contig_reads, contig_snp_off, col_off, col_idx, col_code, win_off, win_start, win_end, label_off, labels, snp_win, grp_off, grp_ids, cell_off, calls;
    hs_recruit_params prm;
};

static hs_recruit_table* part(const Call& k, int c0, int c1) {
    const long long w0 = k.win_off[(size_t)c0], w1 = k.win_off[(size_t)c1];
    const size_t W = (size_t)(w1 - w0);
    std::vector<int32_t> win_contig(W), win_start(W), win_end(W), first(W, 0), last(W, 0);
    for (int c = c0; c < c1; ++c)
        for (long long w = k.win_off[(size_t)c]; w < k.win_off[(size_t)c + 1]; ++w) {
            win_contig[(size_t)(w - w0)] = c - c0; win_start[(size_t)(w - w0)] = (int32_t)k.win_start[(size_t)w]; win_end[(size_t)(w - w0)] = (int32_t)k.win_end[(size_t)w];
        }
    std::vector<int64_t> win_row_off(W + 1, 0);
    std::vector<hs_recruit_row> rows;
    const long long s0 = k.contig_snp_off[(size_t)c0], s1 = k.contig_snp_off[(size_t)c1];
    for (long long w = w0; w < w1; ++w) {
        const long long l0 = k.label_off[(size_t)w], n_reads = k.label_off[(size_t)w + 1] - l0;
        const int32_t G = (int32_t)(k.grp_off[(size_t)w + 1] - k.grp_off[(size_t)w]);
        std::vector<int32_t> ids((size_t)G);
        for (int32_t g = 0; g < G; ++g) ids[(size_t)g] = (int32_t)k.grp_ids[(size_t)k.grp_off[(size_t)w] + (size_t)g];
        // mark
        std::vector<char> flag((size_t)n_reads, 0);
        bool has_snp = false;
        for (long long s = s0; s < s1; ++s) {
            if (k.snp_win[(size_t)s] != w) continue;
            if (!has_snp) { first[(size_t)(w - w0)] = (int32_t)(s - s0); has_snp = true; }
            last[(size_t)(w - w0)] = (int32_t)(s - s0) + 1;
            if (G == 0) continue;
            for (long long e = k.col_off[(size_t)s]; e < k.col_off[(size_t)s + 1]; ++e) {
                const long long r = k.col_idx[(size_t)e];
                if (r >= 0 && r < n_reads && hs::recruit_selected((int32_t)k.labels[(size_t)(l0 + r)], k.prm.which)) flag[(size_t)r] = 1;
            }
        }
        // count: [n_entries, m_0, x_0, m_1, x_1, ...] per row
        std::vector<int64_t> at((size_t)n_reads, -1);
        int64_t words = 0;
        for (long long r = 0; r < n_reads; ++r) if (flag[(size_t)r]) { at[(size_t)r] = words; words += 1 + 2 * (int64_t)G; }
        std::vector<uint32_t> ctr((size_t)words, 0);
        for (long long s = s0; s < s1; ++s) {
            if (k.snp_win[(size_t)s] != w || G == 0) continue;
            for (long long e = k.col_off[(size_t)s]; e < k.col_off[(size_t)s + 1]; ++e) {
                const long long r = k.col_idx[(size_t)e];
                if (r < 0 || r >= n_reads || !flag[(size_t)r]) continue;
                uint32_t* c = ctr.data() + at[(size_t)r];
                c[0] += 1;
                for (int32_t g = 0; g < G; ++g) {
                    const int what = hs::recruit_entry((uint8_t)k.col_code[(size_t)e], (uint8_t)k.calls[(size_t)k.cell_off[(size_t)s] + (size_t)g]);
                    if (what) c[1 + 2 * g + (what - 1)] += 1;
                }
            }
        }
        // decide: groups offered from the last to the first, and in two halves that are merged -- the choice may not depend on the order
        for (long long r = 0; r < n_reads; ++r) {
            if (!flag[(size_t)r]) continue;
            const uint32_t* c = ctr.data() + at[(size_t)r];
            hs::RecruitChoice lo, hi;
            for (int32_t g = G - 1; g >= 0; --g) (g % 2 ? hi : lo).offer(g, c[1 + 2 * g], c[2 + 2 * g]);
            lo.merge(hi);
            rows.push_back(hs::recruit_row(k.prm, (int32_t)r, (int32_t)k.labels[(size_t)(l0 + r)], G, ids.data(), lo, c[0]));
        }
        win_row_off[(size_t)(w - w0) + 1] = (int64_t)rows.size();
    }
    hs::RecruitRaw raw;
    raw.n_windows = (int64_t)W; raw.win_contig = win_contig.data(); raw.win_start = win_start.data(); raw.win_end = win_end.data();
    raw.win_snp_first = first.data(); raw.win_snp_last = last.data(); raw.win_row_off = win_row_off.data(); raw.rows = rows.data();
    raw.contig_base = c0; raw.params = k.prm;
    std::string err;
    hs_recruit_table* t = hs::recruit_assemble(raw, err);
    if (!t) std::fprintf(stderr, "recruit_selftest: %s\n", err.c_str());
    return t;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    std::map<std::string, Arr> j;
    if (!f || !parse(ss.str(), j)) return 2;
    Call k;
    const Arr& p = j["params"];
    if (p.size() != 5 || j["split"].size() != 1) return 2;
    k.prm.which = (int32_t)p[0]; k.prm.min_informative = (int32_t)p[1]; k.prm.min_margin = (int32_t)p[2]; k.prm.mismatch_num = (int32_t)p[3]; k.prm.mismatch_den = (int32_t)p[4];
    if (!hs::recruit_params_valid(k.prm)) return 4;
    k.contig_reads = j["contig_reads"]; k.contig_snp_off = j["contig_snp_off"]; k.col_off = j["col_off"]; k.col_idx = j["col_idx"]; k.col_code = j["col_code"];
    k.win_off = j["win_off"]; k.win_start = j["win_start"]; k.win_end = j["win_end"]; k.label_off = j["label_off"]; k.labels = j["labels"];
    k.snp_win = j["snp_win"]; k.grp_off = j["grp_off"]; k.grp_ids = j["grp_ids"]; k.cell_off = j["cell_off"]; k.calls = j["calls"];
    const int C = (int)k.contig_reads.size(), split = (int)j["split"][0];
    const size_t W = k.win_start.size(), S = k.snp_win.size();
    if (split < 0 || split > C || k.win_off.size() != (size_t)C + 1 || k.contig_snp_off.size() != (size_t)C + 1 || k.label_off.size() != W + 1 || k.grp_off.size() != W + 1 ||
        k.col_off.size() != S + 1 || k.cell_off.size() != S + 1 || k.win_end.size() != W || k.col_idx.size() != k.col_code.size() || (size_t)k.win_off.back() != W ||
        (size_t)k.label_off.back() != k.labels.size() || (size_t)k.col_off.back() != k.col_idx.size() || (size_t)k.cell_off.back() != k.calls.size() ||
        (size_t)k.grp_off.back() != k.grp_ids.size() || (size_t)k.contig_snp_off.back() != S) return 2;
    hs_recruit_table* a = part(k, 0, split);
    hs_recruit_table* b = part(k, split, C);
    if (!a || !b) return 3;
    hs_recruit_table* t = hs::recruit_concat({a, b});
    if (!t) return 3;
    std::vector<std::string> names;
    for (int c = 0; c < C; ++c) names.push_back("c" + std::to_string(c));
    std::vector<const char*> np;
    for (const std::string& s : names) np.push_back(s.c_str());
    char* text = nullptr;
    if (hs_recruit_text(t, np.data(), (int32_t)np.size(), &text)) return 3;
    std::fputs(text, stdout);
    std::free(text);
    std::vector<int32_t> in(k.labels.begin(), k.labels.end()), out(k.labels.size() + 1, 0);
    std::vector<int64_t> label_off(k.label_off.begin(), k.label_off.end());
    if (hs_recruit_apply(t, label_off.data(), in.data(), out.data(), (int64_t)in.size())) return 3;
    std::printf("LABELS\n");
    for (size_t i = 0; i < in.size(); ++i) std::printf("%d ", out[i]);
    std::printf("\nASSIGNED %lld OF %lld IN %lld WINDOWS OF %lld\n", (long long)t->n_assigned, (long long)t->n_rows, (long long)t->n_windows, (long long)t->n_call_windows);
    hs_recruit_table_destroy(a); hs_recruit_table_destroy(b); hs_recruit_table_destroy(t);
    return 0;
}
