"""Inputs for the recruit table (include/hairsplitter_hip.h: hs_recruit_table; kernels in hs_kernels_recruit.hip) built directly in the layout of
tests/allele_cases.py, at the column depths, group counts, label kinds and thresholds where the device takes another route or the rule another branch --
and the rule itself, twice: a dict walk that follows the header's paragraph line by line (recruit_brute) and a vectorised numpy form (recruit_numpy). The
calls of the cells come from allele_cases.rule_brute. Used by tests/test_cpu_recruit_cases.py (the two forms agree, every case reaches its fork, wrong rules
give other tables), tests/test_cpu_recruit_host.py (the host half) and tests/test_gpu_recruit.py (device == recruit_brute).

A case is (contigs, sr, [params, ...]): contigs and sr as in allele_cases, params = dicts of hs_recruit_params. A table is the dict
hairsplitter_amd.api returns (minus its timing fields); "rows" has the dtype ROW."""
import numpy as np

import allele_cases as ac

ROW = np.dtype([("read", "<i4"), ("label", "<i4"), ("best_group", "<i4"), ("second_group", "<i4"), ("m_best", "<u4"), ("x_best", "<u4"),
                ("m_second", "<u4"), ("x_second", "<u4"), ("n_entries", "<u4"), ("assigned", "<i4")])
TABLE_KEYS = ("win_contig", "win_start", "win_end", "win_index", "win_row_off", "rows")
ABSENT, UNCLUSTERED, LABELLED = 1, 2, 4
DEFAULT = {"which": ABSENT | UNCLUSTERED, "min_informative": 3, "min_margin": 2, "mismatch_num": 1, "mismatch_den": 4}
WRONG_RULES = ("tie_assigns", "margin_gt", "informative_gt", "fraction_lt", "undefined_mismatch", "ref_alt_only", "minus1_never", "second_incl_best",
               "dup_once", "clip_index")
# the case (and the index of its params) on which each wrong rule must give another table
WRONG_ON = {"tie_assigns": ("rule", 1), "margin_gt": ("rule", 1), "informative_gt": ("rule", 0), "fraction_lt": ("rule", 0), "undefined_mismatch": ("rule", 1),
            "ref_alt_only": ("rule", 0), "minus1_never": ("which", 1), "second_incl_best": ("rule", 1), "dup_once": ("rule", 0), "clip_index": ("windows", 0)}
REFUSED = ({"min_informative": 0}, {"min_margin": 0}, {"min_margin": -3}, {"mismatch_den": 0}, {"mismatch_num": -1}, {"mismatch_num": 5, "mismatch_den": 4})
BIG = 2 ** 31 - 1


def params(**over):
    return dict(DEFAULT, **over)


def selected(label, which, wrong=None):
    if label >= 0:
        return bool(which & LABELLED)
    if label == -1:
        return bool(which & UNCLUSTERED) and wrong != "minus1_never"
    return label == -2 and bool(which & ABSENT)


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def _windows(contigs, sr):
    """(contig, window index of the call, its SNP columns) for every window that has SNPs: a SNP belongs to the first window that holds it"""
    for c, ctg in enumerate(contigs):
        taken = set()
        for w in range(int(sr["win_off"][c]), int(sr["win_off"][c + 1])):
            lo, hi = int(sr["win_start"][w]), int(sr["win_end"][w])
            mine = [s for s in range(len(ctg["snp_pos"])) if s not in taken and lo <= int(ctg["snp_pos"][s]) <= hi]
            if mine:
                taken.update(mine)
                yield c, w, mine


def _pack(wins, rows, n_call_windows):
    """wins: (contig, start, end, window index, n_rows)"""
    return {"win_contig": np.array([w[0] for w in wins], np.int32), "win_start": np.array([w[1] for w in wins], np.int32),
            "win_end": np.array([w[2] for w in wins], np.int32), "win_index": np.array([w[3] for w in wins], np.int64),
            "win_row_off": np.concatenate(([0], np.cumsum([w[4] for w in wins]))).astype(np.int64),
            "rows": np.array(rows, ROW) if rows else np.zeros(0, ROW), "n_call_windows": n_call_windows}


def recruit_brute(contigs, sr, prm, wrong=None, alleles=None):
    """The header's paragraph, line by line. wrong: one of WRONG_RULES, the rule bent in that one place. Also returns "row_groups" (G of every row)."""
    at = alleles if alleles is not None else ac.rule_brute(contigs, sr)
    wins, rows, row_groups = [], [], []
    for ti, (c, w, mine) in enumerate(_windows(contigs, sr)):
        ctg = contigs[c]
        labels = sr["labels"][int(sr["label_off"][w]):int(sr["label_off"][w + 1])]
        groups = [int(g) for g in at["group_ids"][int(at["win_group_off"][ti]):int(at["win_group_off"][ti + 1])]]
        G = len(groups)
        s0 = int(at["win_snp_off"][ti])
        assert int(at["win_snp_off"][ti + 1]) - s0 == len(mine) and int(at["win_start"][ti]) == int(sr["win_start"][w])
        per_read = {}      # read -> [n_entries, m per group, x per group]
        for j, s in enumerate(mine):
            assert int(at["snp_pos"][s0 + j]) == int(ctg["snp_pos"][s])
            cells = at["cells"][int(at["snp_cell_off"][s0 + j]):int(at["snp_cell_off"][s0 + j]) + G]
            ref, alt = int(ctg["snp_ref"][s]), int(ctg["snp_alt"][s])
            seen = set()
            for e in range(int(ctg["col_off"][s]), int(ctg["col_off"][s + 1])):
                r, code = int(ctg["col_idx"][e]), int(ctg["col_code"][e])
                if wrong == "clip_index" and len(labels):
                    r = min(max(r, 0), len(labels) - 1)
                if not 0 <= r < len(labels):
                    continue      # other indices are ignored
                if G == 0 or not selected(int(labels[r]), prm["which"], wrong):
                    continue      # a window with SNPs but no group has no rows
                if wrong == "dup_once":
                    if r in seen:
                        continue
                    seen.add(r)
                acc = per_read.setdefault(r, [0, [0] * G, [0] * G])
                acc[0] += 1
                for k in range(G):
                    call = int(cells[k]["call"])
                    if call == 0:
                        if wrong == "undefined_mismatch":
                            acc[2][k] += 1
                        continue
                    match = code == call and (wrong != "ref_alt_only" or code in (ref, alt))
                    acc[1 if match else 2][k] += 1
        for r in sorted(per_read):
            n, m, x = per_read[r]
            score = [m[k] - x[k] for k in range(G)]
            best = min(range(G), key=lambda k: (-score[k], k))      # the largest score, the smallest id among equal scores
            others = list(range(G)) if wrong == "second_incl_best" else [k for k in range(G) if k != best]
            second = min(others, key=lambda k: (-score[k], k)) if G > 1 else -1
            inf = m[best] + x[best]
            a_ok = inf > prm["min_informative"] if wrong == "informative_gt" else inf >= prm["min_informative"]
            if G == 1:
                b_ok = True
            else:
                margin = score[best] - score[second]
                b_ok = margin > prm["min_margin"] if wrong == "margin_gt" else margin >= prm["min_margin"]
                if wrong == "tie_assigns" and margin == 0:
                    b_ok = True
            lhs, rhs = x[best] * prm["mismatch_den"], prm["mismatch_num"] * inf
            c_ok = lhs < rhs if wrong == "fraction_lt" else lhs <= rhs
            rows.append((r, int(labels[r]), groups[best], groups[second] if second >= 0 else -1, m[best], x[best], m[second] if second >= 0 else 0,
                         x[second] if second >= 0 else 0, n, int(a_ok and b_ok and c_ok)))
            row_groups.append(G)
        wins.append((c, int(sr["win_start"][w]), int(sr["win_end"][w]), w, len(per_read)))
    t = _pack(wins, rows, len(sr["win_start"]))
    t["row_groups"] = np.array(row_groups, np.int64)
    return t


def recruit_numpy(contigs, sr, prm, alleles=None):
    """the same table with one matrix of matches and one of mismatches per window"""
    at = alleles if alleles is not None else ac.rule_numpy(contigs, sr)
    wins, blocks = [], []
    which = prm["which"]
    for ti, (c, w, mine) in enumerate(_windows(contigs, sr)):
        ctg = contigs[c]
        labels = np.asarray(sr["labels"][int(sr["label_off"][w]):int(sr["label_off"][w + 1])], np.int64)
        g0, g1 = int(at["win_group_off"][ti]), int(at["win_group_off"][ti + 1])
        groups = np.asarray(at["group_ids"][g0:g1], np.int64)
        G, S = len(groups), len(mine)
        s0 = int(at["win_snp_off"][ti])
        off = np.asarray(ctg["col_off"], np.int64)
        ent = np.concatenate([np.arange(off[s], off[s + 1]) for s in mine]) if S else np.zeros(0, np.int64)
        seg = np.repeat(np.arange(S), off[np.array(mine) + 1] - off[np.array(mine)])
        idx = np.asarray(ctg["col_idx"], np.int64)[ent]
        code = np.asarray(ctg["col_code"], np.int64)[ent]
        ok = (idx >= 0) & (idx < len(labels))
        idx, code, seg = idx[ok], code[ok], seg[ok]
        lab = labels[idx] if len(labels) else np.zeros(0, np.int64)
        sel = ((lab >= 0) & bool(which & LABELLED)) | ((lab == -1) & bool(which & UNCLUSTERED)) | ((lab == -2) & bool(which & ABSENT))
        if G == 0:
            sel[:] = False
        idx, code, seg = idx[sel], code[sel], seg[sel]
        reads, inv = np.unique(idx, return_inverse=True)
        R = len(reads)
        rows = np.zeros(R, ROW)
        if R:
            c_off = np.asarray(at["snp_cell_off"], np.int64)[s0:s0 + S]
            calls = np.asarray(at["cells"]["call"], np.int64)[c_off[:, None] + np.arange(G)[None, :]]      # [S, G]
            per = calls[seg]                                                                                    # [E, G]
            match = (per != 0) & (per == code[:, None])
            mis = (per != 0) & ~match
            m = np.zeros((R, G), np.int64); x = np.zeros((R, G), np.int64)
            np.add.at(m, inv, match); np.add.at(x, inv, mis)
            score = m - x
            best = np.argmax(score, axis=1)      # (the first of equal maxima: the smallest slot)
            rr = np.arange(R)
            rows["read"], rows["label"], rows["n_entries"] = reads, labels[reads], np.bincount(inv, minlength=R)
            rows["best_group"], rows["m_best"], rows["x_best"] = groups[best], m[rr, best], x[rr, best]
            inf = m[rr, best] + x[rr, best]
            if G > 1:
                masked = score.copy()
                masked[rr, best] = np.iinfo(np.int64).min
                second = np.argmax(masked, axis=1)
                rows["second_group"], rows["m_second"], rows["x_second"] = groups[second], m[rr, second], x[rr, second]
                b_ok = score[rr, best] - score[rr, second] >= prm["min_margin"]
            else:
                rows["second_group"] = -1
                b_ok = np.ones(R, bool)
            rows["assigned"] = (inf >= prm["min_informative"]) & b_ok & (x[rr, best] * prm["mismatch_den"] <= prm["mismatch_num"] * inf)
        blocks.append(rows)
        wins.append((c, int(sr["win_start"][w]), int(sr["win_end"][w]), w, R))
    t = _pack(wins, [], len(sr["win_start"]))
    t["rows"] = np.concatenate(blocks) if blocks else np.zeros(0, ROW)
    return t


def differences(a, b):
    """the keys in which two tables differ (empty: equal in every field)"""
    out = []
    for k in TABLE_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "rows":
            x, y = x.astype(ROW), y.astype(ROW)
        if x.shape != y.shape or not np.array_equal(x, y):
            out.append(k)
    if int(a["n_call_windows"]) != int(b["n_call_windows"]):
        out.append("n_call_windows")
    return out


def apply_numpy(table, sr):
    """hs_recruit_apply: every assigned row whose old label is < 0 gets its best group"""
    out = np.array(sr["labels"], np.int32, copy=True)
    for w in range(len(table["win_start"])):
        l0 = int(sr["label_off"][int(table["win_index"][w])])
        rows = table["rows"][int(table["win_row_off"][w]):int(table["win_row_off"][w + 1])]
        take = (rows["assigned"] != 0) & (rows["label"] < 0)
        out[l0 + rows["read"][take]] = rows["best_group"][take]
    return out


def text(table, names=None):
    """the text of <outfile>.recruit.tsv"""
    out = []
    for w in range(len(table["win_start"])):
        c = int(table["win_contig"][w])
        out.append("WINDOW\t%s\t%d\t%d\n" % (names[c] if names is not None and 0 <= c < len(names) else str(c), table["win_start"][w], table["win_end"][w]))
        for r in table["rows"][int(table["win_row_off"][w]):int(table["win_row_off"][w + 1])]:
            out.append("READ\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (r["read"], r["label"], r["best_group"], r["m_best"], r["x_best"], r["second_group"],
                                                                            r["m_second"], r["x_second"], r["n_entries"], 1 if r["assigned"] else 0))
    return "".join(out)


def forks(table, prm):
    """what the rows of a brute-force table (with "row_groups") reach, as counters"""
    r, G = table["rows"], table["row_groups"]
    m, x, m2, x2 = (r[k].astype(np.int64) for k in ("m_best", "x_best", "m_second", "x_second"))
    inf, margin = m + x, (m - x) - (m2 - x2)
    multi = G > 1
    a_ok, c_ok = inf >= prm["min_informative"], x * prm["mismatch_den"] <= prm["mismatch_num"] * inf
    return {"rows": len(r), "assigned": int((r["assigned"] != 0).sum()), "wide": int((G > 64).sum()), "lane": int((G <= 64).sum()), "one_group": int((G == 1).sum()),
            "tie": int((multi & (margin == 0)).sum()), "tie_otherwise_fine": int((multi & (margin == 0) & a_ok & c_ok).sum()),
            "margin_at_min": int((multi & (margin == prm["min_margin"]) & a_ok & c_ok).sum()),
            "margin_below_min": int((multi & (margin == prm["min_margin"] - 1) & a_ok & c_ok).sum()),
            "informative_at_min": int(((inf == prm["min_informative"]) & (r["assigned"] != 0)).sum()),
            "informative_below_min": int((inf == prm["min_informative"] - 1).sum()),
            "fraction_exact": int(((x * prm["mismatch_den"] == prm["mismatch_num"] * inf) & (x > 0) & (r["assigned"] != 0)).sum()),
            "fraction_alone_refuses": int((a_ok & (~multi | (margin >= prm["min_margin"])) & ~c_ok).sum()),
            "negative_best": int((m - x < 0).sum()), "empty_best": int((inf == 0).sum()),
            "labelled_own": int(((r["label"] >= 0) & (r["label"] == r["best_group"])).sum()),
            "labelled_other": int(((r["label"] >= 0) & (r["label"] != r["best_group"])).sum()),
            "absent": int((r["label"] == -2).sum()), "unclustered": int((r["label"] == -1).sum()),
            "entries_differ": int((r["n_entries"].astype(np.int64) != inf).sum())}


# ------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------
REF, ALT, THIRD = 40, 47, 52


def scene(windows, core=5, length=1000):
    """One contig, one window of `length` bases per entry of `windows` = (n_snps, {group id: [code per SNP; 0 = an undefined call]}, [(label, {snp: code or
    [codes]}), ...]): `core` reads per group carry the group's code at every SNP (five different codes where the call shall be undefined); the extra reads
    follow them in the read order, with the label and the entries given (a list of codes: the read stands that often in the column)."""
    n_reads = max(core * len(g) + len(extra) for _, g, extra in windows)
    cols, wins, labels = [], [], []
    for k, (n_snps, groups, extra) in enumerate(windows):
        lab = np.full(n_reads, -2, np.int32)
        for gi, g in enumerate(groups):
            lab[core * gi:core * (gi + 1)] = g
        first = core * len(groups)
        for i, (label, _) in enumerate(extra):
            lab[first + i] = label
        for j in range(n_snps):
            ids, codes = [], []
            for gi, (g, gc) in enumerate(groups.items()):
                for i in range(core):
                    ids.append(core * gi + i)
                    codes.append(gc[j] if gc[j] else (40, 47, 52, 61, 70)[i % 5])
            for i, (_, ent) in enumerate(extra):
                for code in ([] if j not in ent else ent[j] if isinstance(ent[j], list) else [ent[j]]):
                    ids.append(first + i); codes.append(code)
            cols.append([length * k + 10 * (j + 1), REF, ALT, ids, codes])
        wins.append((length * k, length * k + length - 1)); labels.append(lab)
    ctg = raw_contig(n_reads, length * len(windows), cols)
    return [ctg], ac.result([ctg], [wins], [labels])


def raw_contig(n_reads, length, columns, pad=0):
    """allele_cases.contig without its checks: read indices may repeat, descend or lie outside [0, n_reads)"""
    off, idx, code = [pad], [np.zeros(pad, np.int32)], [np.full(pad, 35, np.uint8)]
    for _, _, _, ids, codes in columns:
        assert len(ids) == len(codes) <= 65535
        idx.append(np.asarray(ids, np.int32)); code.append(np.asarray(codes, np.uint8)); off.append(off[-1] + len(ids))
    return {"length": int(length), "read_start": np.zeros(n_reads, np.int32), "read_end": np.full(n_reads, length, np.int32),
            "snp_pos": np.array([c[0] for c in columns], np.int32), "snp_ref": np.array([c[1] for c in columns], np.uint8),
            "snp_alt": np.array([c[2] for c in columns], np.uint8), "col_off": np.array(off, np.int64),
            "col_idx": np.concatenate(idx).astype(np.int32), "col_code": np.concatenate(code).astype(np.uint8)}


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
DEPTHS = (1, 63, 64, 65, 128, 129, 4097)


def case_depth():
    """one window, groups {0, 3}; columns of DEPTHS entries, one of rows' entries only (its cells have no entry: every call undefined), one of labelled reads
    only, an empty one. Every fourth read is absent (-2), every fifth unclustered (-1)."""
    rng = np.random.default_rng(15)
    n = 4300
    labels = np.array([0, 3], np.int32)[rng.integers(0, 2, n)]
    labels[::4] = -2
    labels[::5] = -1
    own = np.where(labels == 3, ALT, REF)
    loose = np.flatnonzero(labels < 0)
    own[loose] = np.where(rng.random(len(loose)) < 0.5, REF, ALT)      # a leftover read follows one group or the other
    cols = []
    for k, d in enumerate(DEPTHS):
        ids = np.sort(rng.permutation(n)[:d]) if d > 1 else loose[7:8]
        noisy = np.where(rng.random(d) < 0.1, THIRD, own[ids])
        cols.append((100 + 10 * k, REF, ALT, ids, noisy))
    rows_only = np.sort(rng.permutation(loose)[:70])
    cols.append((300, REF, ALT, rows_only, own[rows_only]))
    none = np.sort(rng.permutation(np.flatnonzero(labels >= 0))[:70])
    cols.append((310, REF, ALT, none, own[none]))
    cols.append((320, REF, ALT, np.zeros(0, np.int64), np.zeros(0, np.uint8)))
    ctgs = [ac.contig(n, 3000, cols)]
    return ctgs, ac.result(ctgs, [[(0, 2999)]], [[labels]]), [params()]


GROUP_SIZES = (1, 2, 63, 64, 0, 65, 300)
GROUP_SNPS = 10


def case_groups():
    """windows of G = GROUP_SIZES groups of ONE read each (ids 0, 3, 6, ... and LARGE_ID; group k carries the bits of k over ten SNPs, so no two groups
    call alike), behind them 20 reads without a label: the odd ones stand in all ten columns with the pattern of one group (a unique best, the runner-up one
    bit away), the even ones in the first three only (many groups tie: the smallest id is best, the next one second). G = 0: SNPs and no group, no rows."""
    n = max(GROUP_SIZES) + 20
    cols, wins, labels = [], [], []
    for k, G in enumerate(GROUP_SIZES):
        lab = np.full(n, -2, np.int32)
        ids = (3 * np.arange(G)).astype(np.int64)
        if G > 1:
            ids[-1] = ac.LARGE_ID
        lab[:G] = ids
        loose = np.arange(max(GROUP_SIZES), n)
        lab[loose[::3]] = -1
        follows = (loose * 7 + 3) % max(G, 1)
        for j in range(GROUP_SNPS):
            bit = lambda v: np.where((v >> j) & 1, ALT, REF)
            there = loose[(loose % 2 == 1) | (j < 3)]
            cols.append((1000 * k + 10 * (j + 1), REF, ALT, np.concatenate((np.arange(G), there)), np.concatenate((bit(np.arange(G)), bit(follows[there - loose[0]])))))
        labels.append(lab); wins.append((1000 * k, 1000 * k + 999))
    ctgs = [ac.contig(n, 1000 * len(GROUP_SIZES), cols)]
    return ctgs, ac.result(ctgs, [wins], [labels]), [params()]


def _rule_scene():
    """two groups, 0 (calls REF) and 5 (calls ALT), eight SNPs: at SNP 6 group 5 has no call, at SNP 7 group 0 calls THIRD. The extra reads, in order:"""
    A = [REF] * 6 + [REF, THIRD]
    B = [ALT] * 6 + [0, ALT]
    extra = [(-2, {0: REF, 1: REF}),                                  # 0 informative = min - 1
             (-2, {0: REF, 1: REF, 2: REF}),                          # 1 informative = min, no mismatch
             (-2, {0: REF, 1: ALT, 6: REF}),                          # 2 margin 1 = min - 1 (SNP 6 counts for group 0 only)
             (-2, {0: REF, 1: REF, 2: ALT}),                          # 3 margin 2 = min, fraction 1/3
             (-2, {0: REF, 1: ALT, 2: REF, 3: ALT}),                  # 4 margin 0: a tie, the smaller id reported, never assigned
             (-2, {0: REF, 1: REF, 2: REF, 3: ALT}),                  # 5 fraction exactly 1/4
             (-2, {0: REF, 1: REF, 2: REF, 3: ALT, 4: ALT}),          # 6 one mismatch above: 2/5, margin still 2
             (-2, {0: THIRD, 1: THIRD, 6: THIRD}),                    # 7 scores -3 and -2: a negative score that is the best
             (-2, {6: THIRD}),                                        # 8 group 5 has m = x = 0 (its only call undefined) and is the best, score 0 over -1
             (-2, {7: THIRD, 0: REF, 1: REF}),                        # 9 THIRD is neither ref nor alt and equals the call of group 0
             (-2, {0: [REF, REF], 1: REF}),                           # 10 twice in one column: informative 3 only with the duplicate
             (-1, {0: ALT, 1: ALT, 2: ALT}),                          # 11 unclustered, fits group 5
             (0, {0: REF, 1: REF, 2: REF}),                           # 12 labelled 0, best group its own
             (0, {0: ALT, 1: ALT, 2: ALT}),                           # 13 labelled 0, best group the other one
             (5, {0: ALT, 1: ALT, 2: ALT, 3: ALT})]                   # 14 labelled 5, its own
    return scene([(8, {0: A, 5: B}, extra)])


def case_rule():
    """every branch of the choice and of (a), (b), (c) on the reads of _rule_scene, under 1/4, 1/1, 0/1 and (2^31 - 1)/(2^31 - 1)"""
    ctgs, sr = _rule_scene()
    return ctgs, sr, [params(), params(mismatch_num=1, mismatch_den=1), params(mismatch_num=0, mismatch_den=1), params(mismatch_num=BIG, mismatch_den=BIG)]


def case_which():
    """each bit alone and all three together, on the reads of _rule_scene"""
    ctgs, sr = _rule_scene()
    return ctgs, sr, [params(which=ABSENT), params(which=UNCLUSTERED), params(which=LABELLED), params(which=ABSENT | UNCLUSTERED | LABELLED)]


def case_windows():
    """five contigs. 0: SNPs at win_start and win_end, a window without SNPs between two that have some, a SNP behind the last window, col_off not from 0; every
    read without a label in one window has rows in the others too. 1: no SNPs. 2: no windows. 3: no reads (a window and a SNP with an empty column). 4: one
    window whose columns also hold the read indices -1 and n_reads (ignored; clipped they would add entries to the first and the last read, both rows)."""
    rng = np.random.default_rng(18)
    n = 24
    lab = lambda: np.array([0, 1, 4, -1, -2], np.int32)[rng.integers(0, 5, n)]
    follow = np.where(rng.random(n) < 0.5, REF, ALT)
    col = lambda pos: (pos, REF, ALT, np.arange(n), np.where(rng.random(n) < 0.9, follow, THIRD))
    c0 = ac.contig(n, 3700, [col(0), col(499), col(1000), col(1001), col(1002), col(2600), col(2601), col(2602), col(3650)], pad=7)
    w0 = [(0, 499), (500, 999), (1000, 1499), (1500, 3600)]
    c1 = ac.contig(5, 900, [])
    c2 = ac.contig(6, 900, [(10, REF, ALT, np.arange(6), np.full(6, REF))])
    c3 = ac.contig(0, 900, [(10, REF, ALT, np.zeros(0, np.int64), np.zeros(0, np.uint8))])
    l4 = np.array([-2] + [0] * 5 + [1] * 5 + [-1], np.int32)
    code4 = np.array([REF] + [REF] * 5 + [ALT] * 5 + [ALT], np.uint8)
    n4 = len(l4)
    c4 = raw_contig(n4, 800, [(100 + 10 * j, REF, ALT, np.concatenate(([-1], np.arange(n4), [n4])), np.concatenate(([ALT], code4, [REF]))) for j in range(4)])
    ctgs = [c0, c1, c2, c3, c4]
    sr = ac.result(ctgs, [w0, [(0, 899)], [], [(0, 899)], [(0, 799)]], [[lab() for _ in w0], [np.zeros(5, np.int32)], [], [np.zeros(0, np.int32)], [l4]])
    return ctgs, sr, [params()]


def case_empty():
    """no contigs at all"""
    ctgs, sr = ac.case_empty()
    return ctgs, sr, [params()]


CASES = {"depth": case_depth, "groups": case_groups, "which": case_which, "rule": case_rule, "windows": case_windows, "empty": case_empty}


def get(name):
    return CASES[name]()


def host_input(contigs, sr, prm, split):
    """what tests/harness/recruit_selftest.cpp reads: the call as flat integer arrays -- columns, dense labels, and the allele plan with the calls of its
    cells as the kernels get them (over EVERY window and SNP of the call) --, one JSON object"""
    import json
    at = ac.rule_brute(contigs, sr)
    W = len(sr["win_start"])
    snp_base = np.concatenate(([0], np.cumsum([len(c["snp_pos"]) for c in contigs]))).astype(np.int64)
    S = int(snp_base[-1])
    snp_win = np.full(S, -1, np.int64)
    grp = [[] for _ in range(W)]
    calls = [[] for _ in range(S)]
    for ti, (c, w, mine) in enumerate(_windows(contigs, sr)):
        grp[w] = [int(g) for g in at["group_ids"][int(at["win_group_off"][ti]):int(at["win_group_off"][ti + 1])]]
        for j, s in enumerate(mine):
            o = int(at["snp_cell_off"][int(at["win_snp_off"][ti]) + j])
            snp_win[snp_base[c] + s] = w
            calls[snp_base[c] + s] = [int(v) for v in at["cells"]["call"][o:o + len(grp[w])]]
    depth = [int(c["col_off"][s + 1] - c["col_off"][s]) for c in contigs for s in range(len(c["snp_pos"]))]
    flat = lambda key: [int(v) for c in contigs for v in c[key][int(c["col_off"][0]):int(c["col_off"][-1])]]
    ints = lambda a: [int(v) for v in a]
    cum = lambda n: ints(np.concatenate(([0], np.cumsum(n))))
    return json.dumps({"params": [prm[k] for k in ("which", "min_informative", "min_margin", "mismatch_num", "mismatch_den")], "split": [split],
                       "contig_reads": [len(c["read_start"]) for c in contigs], "contig_snp_off": ints(snp_base), "col_off": cum(depth),
                       "col_idx": flat("col_idx"), "col_code": flat("col_code"), "win_off": ints(sr["win_off"]), "win_start": ints(sr["win_start"]),
                       "win_end": ints(sr["win_end"]), "label_off": ints(sr["label_off"]), "labels": ints(sr["labels"]), "snp_win": ints(snp_win),
                       "grp_off": cum([len(g) for g in grp]), "grp_ids": [g for gs in grp for g in gs], "cell_off": cum([len(x) for x in calls]),
                       "calls": [v for x in calls for v in x]})
