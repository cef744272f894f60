"""Inputs for the allele table (include/hairsplitter_hip.h: hs_allele_table; kernels in hs_kernels_alleles.hip) built directly, at the column depths, group
counts, code counts and window layouts where the device takes another route or the rule takes another branch -- and the rule itself, twice: a per-cell
dict walk that follows the header's paragraph line by line (rule_brute) and a vectorised numpy form (rule_numpy). Used by tests/test_cpu_allele_cases.py
(the two forms agree, every case reaches its fork, deliberately wrong rules give other tables) and tests/test_gpu_alleles.py (device == rule_brute).

A case is (contigs, sr): contigs = one dict per contig as hairsplitter_amd.api.haplotype_alleles takes them (length, read_start, read_end, snp_pos, snp_ref,
snp_alt, col_off, col_idx, col_code), sr = {"win_off", "win_start", "win_end", "label_off", "labels"} in the layout of a stage-4 result. A table is the
dict hairsplitter_amd.api returns (minus its timing fields); "cells" has the dtype CELL."""
import numpy as np

CELL = np.dtype([("n", "<u2"), ("best", "<u2"), ("second", "<u2"), ("n_ref", "<u2"), ("n_alt", "<u2"), ("best_code", "u1"), ("call", "u1")])
TABLE_KEYS = ("win_contig", "win_start", "win_end", "win_group_off", "group_ids", "win_snp_off", "snp_contig", "snp_pos", "snp_ref", "snp_alt", "snp_n_calls",
              "snp_cell_off", "cells")
CODES = np.arange(33, 158, dtype=np.uint8)      # the 125 pileup codes
WRONG_RULES = ("second_ge", "n_ge", "tie_largest", "minus1_group", "pos_lt_end", "second_distinct")
LARGE_ID = 2 ** 31 - 2                          # the largest label a window may carry


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def _pack(wins, snps, cells):
    """wins: (contig, start, end, [group ids], n_snps); snps: (contig, pos, ref, alt, n_calls); cells: tuples in CELL order, SNP by SNP"""
    t = {"win_contig": np.array([w[0] for w in wins], np.int32), "win_start": np.array([w[1] for w in wins], np.int32),
         "win_end": np.array([w[2] for w in wins], np.int32),
         "win_group_off": np.concatenate(([0], np.cumsum([len(w[3]) for w in wins]))).astype(np.int64),
         "group_ids": np.array([g for w in wins for g in w[3]], np.int32),
         "win_snp_off": np.concatenate(([0], np.cumsum([w[4] for w in wins]))).astype(np.int64),
         "snp_contig": np.array([s[0] for s in snps], np.int32), "snp_pos": np.array([s[1] for s in snps], np.int32),
         "snp_ref": np.array([s[2] for s in snps], np.uint8), "snp_alt": np.array([s[3] for s in snps], np.uint8),
         "snp_n_calls": np.array([s[4] for s in snps], np.int32)}
    per_snp = np.repeat(np.diff(t["win_group_off"]), np.diff(t["win_snp_off"]))
    t["snp_cell_off"] = np.concatenate(([0], np.cumsum(per_snp))).astype(np.int64)
    t["cells"] = np.array(cells, CELL) if cells else np.zeros(0, CELL)
    return t


def _windows_of(sr, c):
    return range(int(sr["win_off"][c]), int(sr["win_off"][c + 1]))


def rule_brute(contigs, sr, wrong=None):
    """The header's paragraph, line by line. wrong: one of WRONG_RULES, the rule bent in that one place."""
    wins, snps, cells = [], [], []
    for c, ctg in enumerate(contigs):
        taken = set()      # every SNP falls in exactly one window: the first that holds it
        for w in _windows_of(sr, c):
            labels = sr["labels"][int(sr["label_off"][w]):int(sr["label_off"][w + 1])]
            lo, hi = int(sr["win_start"][w]), int(sr["win_end"][w])
            floor = -1 if wrong == "minus1_group" else 0
            groups = sorted({int(x) for x in labels if x >= floor})      # the distinct labels >= 0, ascending, ids kept
            mine = [s for s in range(len(ctg["snp_pos"]))
                    if s not in taken and lo <= int(ctg["snp_pos"][s]) and (int(ctg["snp_pos"][s]) < hi if wrong == "pos_lt_end" else int(ctg["snp_pos"][s]) <= hi)]
            if not mine:
                continue      # windows without SNPs contribute nothing
            taken.update(mine)
            wins.append((c, lo, hi, groups, len(mine)))
            for s in mine:
                ref, alt = int(ctg["snp_ref"][s]), int(ctg["snp_alt"][s])
                a, b = int(ctg["col_off"][s]), int(ctg["col_off"][s + 1])
                calls = set()
                for g in groups:
                    count = {}      # over the column entries whose read has that label in that window
                    for e in range(a, b):
                        r = int(ctg["col_idx"][e])
                        if 0 <= r < len(labels) and int(labels[r]) == g:
                            code = int(ctg["col_code"][e])
                            count[code] = count.get(code, 0) + 1
                    n = sum(count.values())
                    by_count = sorted(count.values(), reverse=True)
                    best = by_count[0] if by_count else 0
                    if wrong == "second_distinct":
                        rest = sorted(set(by_count), reverse=True)
                        second = rest[1] if len(rest) > 1 else 0
                    else:
                        second = by_count[1] if len(by_count) > 1 else 0      # two codes tied at the top: second == best
                    at_best = [k for k, v in count.items() if v == best]
                    best_code = (max(at_best) if wrong == "tie_largest" else min(at_best)) if at_best else 0
                    undefined = n == 0 or (2 * second >= best if wrong == "second_ge" else 2 * second > best) or (n >= 2 * best if wrong == "n_ge" else n > 2 * best)
                    call = 0 if undefined else best_code
                    if call:
                        calls.add(call)
                    cells.append((n, best, second, count.get(ref, 0), count.get(alt, 0), best_code, call))
                snps.append((c, int(ctg["snp_pos"][s]), ref, alt, len(calls)))
    return _pack(wins, snps, cells)


def rule_numpy(contigs, sr):
    """the same table from sorted (cell, code) keys, one window at a time"""
    wins, snps, cell_blocks = [], [], []
    for c, ctg in enumerate(contigs):
        pos = np.asarray(ctg["snp_pos"], np.int64)
        off = np.asarray(ctg["col_off"], np.int64)
        taken = np.zeros(len(pos), bool)
        for w in _windows_of(sr, c):
            labels = np.asarray(sr["labels"][int(sr["label_off"][w]):int(sr["label_off"][w + 1])], np.int64)
            lo, hi = int(sr["win_start"][w]), int(sr["win_end"][w])
            mine = np.flatnonzero(~taken & (pos >= lo) & (pos <= hi))
            if len(mine) == 0:
                continue
            taken[mine] = True
            groups = np.unique(labels[labels >= 0])
            G, S = len(groups), len(mine)
            wins.append((c, lo, hi, groups.tolist(), S))
            cells = np.zeros(S * G, CELL)
            n_calls = np.zeros(S, np.int64)
            depth = off[mine + 1] - off[mine]
            if G and depth.sum():
                seg = np.repeat(np.arange(S), depth)
                ent = np.concatenate([np.arange(off[s], off[s + 1]) for s in mine])
                idx = np.asarray(ctg["col_idx"], np.int64)[ent]
                code = np.asarray(ctg["col_code"], np.int64)[ent]
                known = (idx >= 0) & (idx < len(labels))
                lab = np.where(known, labels[np.clip(idx, 0, max(len(labels) - 1, 0))] if len(labels) else -2, -2)
                ok = lab >= 0
                seg, code, lab = seg[ok], code[ok], lab[ok]
                cell = seg * G + np.searchsorted(groups, lab)
                key, cnt = np.unique(cell * 256 + code, return_counts=True)
                kc, kcode = key // 256, key % 256
                order = np.lexsort((kcode, -cnt, kc))      # inside a cell: largest count first, smallest code first among equals
                kc, kcode, cnt = kc[order], kcode[order], cnt[order]
                first = np.flatnonzero(np.concatenate(([True], kc[1:] != kc[:-1])))
                cid = kc[first]
                n = np.add.reduceat(cnt, first)
                best, best_code = cnt[first], kcode[first]
                nxt = first + 1
                has2 = (nxt < len(kc)) & (kc[np.minimum(nxt, len(kc) - 1)] == cid)
                second = np.where(has2, cnt[np.minimum(nxt, len(kc) - 1)], 0)
                ref = np.asarray(ctg["snp_ref"], np.int64)[mine][kc // G]
                alt = np.asarray(ctg["snp_alt"], np.int64)[mine][kc // G]
                n_ref = np.bincount(kc, weights=cnt * (kcode == ref), minlength=S * G).astype(np.int64)
                n_alt = np.bincount(kc, weights=cnt * (kcode == alt), minlength=S * G).astype(np.int64)
                call = np.where((2 * second > best) | (n > 2 * best), 0, best_code)
                cells["n"][cid], cells["best"][cid], cells["second"][cid] = n, best, second
                cells["best_code"][cid], cells["call"][cid] = best_code, call
                cells["n_ref"], cells["n_alt"] = n_ref, n_alt
                called = np.unique((cid // G) * 256 + call)
                called = called[called % 256 != 0]
                n_calls = np.bincount(called // 256, minlength=S)
            cell_blocks.append(cells)
            for k, s in enumerate(mine):
                snps.append((c, int(pos[s]), int(ctg["snp_ref"][s]), int(ctg["snp_alt"][s]), int(n_calls[k])))
    t = _pack(wins, snps, [])
    t["cells"] = np.concatenate(cell_blocks) if cell_blocks else np.zeros(0, CELL)
    return t


def differences(a, b):
    """the keys in which two tables differ (empty: equal in every field)"""
    out = []
    for k in TABLE_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "cells":
            x, y = x.astype(CELL), y.astype(CELL)
        if x.shape != y.shape or not np.array_equal(x, y):
            out.append(k)
    return out


# ------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------
def contig(n_reads, length, columns, pad=0):
    """columns: (pos, ref, alt, read ids, codes) in ascending position; pad: entries in front of the first column (col_off does not start at 0)"""
    off, idx, code = [pad], [np.zeros(pad, np.int32)], [np.full(pad, 35, np.uint8)]
    for _, _, _, ids, codes in columns:
        ids = np.asarray(ids, np.int32)
        assert len(ids) == len(codes) and np.all(np.diff(ids) > 0) and (len(ids) == 0 or (ids[0] >= 0 and ids[-1] < n_reads)) and len(ids) <= 65535
        idx.append(ids); code.append(np.asarray(codes, np.uint8)); off.append(off[-1] + len(ids))
    return {"length": int(length), "read_start": np.zeros(n_reads, np.int32), "read_end": np.full(n_reads, length, np.int32),
            "snp_pos": np.array([c[0] for c in columns], np.int32), "snp_ref": np.array([c[1] for c in columns], np.uint8),
            "snp_alt": np.array([c[2] for c in columns], np.uint8), "col_off": np.array(off, np.int64),
            "col_idx": np.concatenate(idx).astype(np.int32), "col_code": np.concatenate(code).astype(np.uint8)}


def result(contigs, windows, labels):
    """windows[c] = [(start, end), ...]; labels[c][k] = the labels of window k of contig c, one per read of the contig"""
    win_off, ws, we, lo, lab = [0], [], [], [0], []
    for c, ctg in enumerate(contigs):
        for k, (a, b) in enumerate(windows[c]):
            row = np.asarray(labels[c][k], np.int32)
            assert len(row) == len(ctg["read_start"])
            ws.append(a); we.append(b); lab.append(row); lo.append(lo[-1] + len(row))
        win_off.append(len(ws))
    return {"win_off": np.array(win_off, np.int64), "win_start": np.array(ws, np.int32), "win_end": np.array(we, np.int32),
            "label_off": np.array(lo, np.int64), "labels": np.concatenate(lab).astype(np.int32) if lab else np.zeros(0, np.int32)}


def column_from_counts(pos, ref, alt, group_reads, counts):
    """counts = {group: {code: count}}: the first reads of every group carry the codes, in code order; its other reads are not in the column"""
    ids, codes = [], []
    for g, cc in counts.items():
        reads = group_reads[g]
        need = sum(cc.values())
        assert need <= len(reads), (g, need, len(reads))
        ids.extend(reads[:need])
        for code, k in sorted(cc.items()):
            codes.extend([code] * k)
    order = np.argsort(ids)
    return (pos, ref, alt, np.asarray(ids)[order], np.asarray(codes)[order])


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def case_depths(lds_cap):
    """one window; columns of 1, 63, 64, 65, 255, 256 entries and of lds_cap and lds_cap + 1 (the first column the LDS route hands on). Groups {0, 3, 7};
    every tenth read is unclustered (-1), every eleventh absent from the window (-2): both sit inside every deep column."""
    rng = np.random.default_rng(5)
    n = lds_cap + 40
    labels = np.array([0, 3, 7], np.int32)[rng.integers(0, 3, n)]
    labels[::10] = -1
    labels[::11] = -2
    cols = []
    for k, d in enumerate((1, 63, 64, 65, 255, 256, lds_cap, lds_cap + 1)):
        ids = np.sort(rng.permutation(n)[:d]) if d > 1 else np.array([5])
        cols.append((100 + 10 * k, 40, 47, ids, np.array([40, 47, 52, 90], np.uint8)[rng.integers(0, 4, d) % (2 + k % 3)]))
    ctgs = [contig(n, 3000, cols)]
    return ctgs, result(ctgs, [[(0, 2999)]], [[labels]])


def case_groups():
    """windows with 1, 2, 63, 64, 65 and 300 groups, ids that are not 0..G-1 (every id times three, one LARGE_ID), and a window with no label >= 0 between
    them; two SNPs per window, every group on the first, every second one on the other"""
    sizes = (1, 2, 63, 64, 0, 65, 300)
    n = 2 * max(sizes) + 7
    rng = np.random.default_rng(6)
    cols, wins, labels = [], [], []
    for k, G in enumerate(sizes):
        lab = np.full(n, -1, np.int32)
        ids = (3 * np.arange(G)).astype(np.int64)
        if G > 1:
            ids[-1] = LARGE_ID
        lab[:2 * G] = np.repeat(ids, 2).astype(np.int32)[rng.permutation(2 * G)] if G else lab[:0]
        lab[-3:] = -2
        labels.append(lab); wins.append((1000 * k, 1000 * k + 999))
        every = np.arange(n)
        cols.append((1000 * k + 10, 33, 58, every, np.where(rng.random(n) < 0.8, 33, 58)))
        half = np.arange(0, n, 2)
        cols.append((1000 * k + 500, 70, 71, half, np.where(rng.random(len(half)) < 0.5, 70, 71)))
    ctgs = [contig(n, 1000 * len(sizes), cols)]
    return ctgs, result(ctgs, [wins], [labels])


CODE_SCENARIOS = {      # one SNP each: {group: {code: count}} with ref = 40, alt = 47
    "tie_top": {0: {40: 5, 47: 5}, 1: {47: 9}},
    "tie_second": {0: {40: 10, 47: 2, 52: 2}, 1: {40: 3}},
    "second_half_of_best": {0: {40: 10, 47: 5}, 1: {47: 12, 40: 6}},
    "second_above_half": {0: {40: 11, 47: 6}, 1: {47: 4}},
    "n_twice_best": {0: {40: 6, 47: 2, 52: 2, 61: 2}, 1: {47: 7}},
    "n_above_twice_best": {0: {40: 6, 47: 2, 52: 2, 61: 2, 77: 1}, 1: {47: 7}},
    "five_codes": {0: {40: 30, 47: 3, 52: 3, 61: 2, 77: 1, 90: 1}, 1: {40: 1}},
    "all_codes": {0: {int(c): 1 + (c == 33) for c in CODES}, 1: {47: 2}},
    "ref_absent": {0: {47: 8, 52: 1}, 1: {40: 8}},
    "alt_absent": {0: {40: 8}, 1: {40: 7, 52: 2}},
    "group_absent": {1: {47: 8}},
}


def case_codes():
    """one window, groups 0 and 1 (and the unclustered), one SNP per entry of CODE_SCENARIOS"""
    n0, n1 = 130, 20
    labels = np.concatenate((np.zeros(n0, np.int32), np.ones(n1, np.int32), np.full(5, -1, np.int32)))
    reads = {0: list(range(n0)), 1: list(range(n0, n0 + n1))}
    cols = [column_from_counts(50 + 20 * k, 40, 47, reads, sc) for k, sc in enumerate(CODE_SCENARIOS.values())]
    ctgs = [contig(len(labels), 2000, cols)]
    return ctgs, result(ctgs, [[(0, 1999)]], [[labels]])


def case_labels():
    """entries labelled -1 and -2 inside a column that would change the call if they counted, and a column entry whose read the window does not hold (-2 there,
    a group in the next window)"""
    lab_a = np.array([0] * 6 + [1] * 6 + [-1] * 9 + [-2] * 9, np.int32)
    lab_b = np.array([0] * 6 + [1] * 6 + [2] * 9 + [-1] * 9, np.int32)      # the reads absent from window a form group 2 in window b
    n = len(lab_a)
    code = np.array([40] * 6 + [47] * 6 + [52] * 9 + [61] * 9, np.uint8)
    cols = [(100, 40, 47, np.arange(n), code), (1100, 40, 47, np.arange(n), code)]
    ctgs = [contig(n, 2000, cols)]
    return ctgs, result(ctgs, [[(0, 999), (1000, 1999)]], [[lab_a, lab_b]])


def case_windows():
    """three contigs and one more. 0: SNPs at win_start and win_end, a window without SNPs between two that have some, a terminal window longer than the others,
    a SNP behind the last window (in no window); its col_off does not start at 0. 1: no SNPs. 2: no windows (its SNP is in no table). 3: one plain window."""
    rng = np.random.default_rng(8)
    n = 24
    lab = lambda: np.array([0, 1, 4, -1], np.int32)[rng.integers(0, 4, n)]
    col = lambda pos: (pos, 40, 47, np.arange(n), np.where(rng.random(n) < 0.5, 40, 47))
    c0 = contig(n, 3700, [col(0), col(499), col(1000), col(1001), col(2600), col(3650)], pad=7)
    w0 = [(0, 499), (500, 999), (1000, 1499), (1500, 3600)]
    c1 = contig(5, 900, [])
    c2 = contig(6, 900, [(10, 40, 47, np.arange(6), np.full(6, 40))])
    c3 = contig(n, 800, [col(300)])
    ctgs = [c0, c1, c2, c3]
    return ctgs, result(ctgs, [w0, [(0, 899)], [], [(0, 799)]], [[lab() for _ in w0], [np.zeros(5, np.int32)], [], [lab()]])


WIDE_COLUMNS = 70       # more columns beyond the LDS route than the kernel behind it has workgroups (64): some workgroup takes a second one


def case_deepest(lds_cap):
    """the path's deepest column, 65535 entries, and WIDE_COLUMNS columns one entry past the LDS route; groups {2, 5, 6}, a few reads unclustered"""
    rng = np.random.default_rng(9)
    n = 65535
    labels = np.array([2, 5, 6, -1], np.int32)[rng.integers(0, 4, n)]
    cols = [(10, 40, 47, np.arange(n), np.array([40, 47, 52], np.uint8)[rng.integers(0, 3, n)])]
    for k in range(WIDE_COLUMNS):
        ids = np.sort(rng.permutation(n)[:lds_cap + 1])
        cols.append((20 + k, 40, 47, ids, np.where(labels[ids] == 5, 47, 40).astype(np.uint8)))
    ctgs = [contig(n, 1000, cols)]
    return ctgs, result(ctgs, [[(0, 999)]], [[labels]])


def case_empty():
    """no contigs at all"""
    return [], result([], [], [])


CASES = {"depths": case_depths, "groups": case_groups, "codes": case_codes, "labels": case_labels, "windows": case_windows, "empty": case_empty,
         "deepest": case_deepest}


def get(name, lds_cap=2048):
    return CASES[name](lds_cap) if name in ("depths", "deepest") else CASES[name]()
