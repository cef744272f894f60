"""tests/recruit_cases.py without a device: the two statements of the rule agree on every case, every case reaches the fork it is there for (asserted on
counters derived from the case itself), a rule bent in one place gives another table on the case aimed at that place, and hs_recruit_apply stated in numpy
is what the host half of the library does (tests/harness/recruit_selftest.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import recruit_cases as rc

RUNS = [(name, i) for name in sorted(rc.CASES) for i in range(len(rc.get(name)[2]))]


@pytest.fixture(scope="module")
def cases():
    return {name: rc.get(name) for name in rc.CASES}


@pytest.fixture(scope="module")
def tables(cases):
    return {(name, i): rc.recruit_brute(cases[name][0], cases[name][1], cases[name][2][i]) for name, i in RUNS}


@pytest.mark.parametrize("name,i", RUNS)
def test_the_two_forms_agree(cases, tables, name, i):
    ctgs, sr, prms = cases[name]
    assert rc.differences(tables[(name, i)], rc.recruit_numpy(ctgs, sr, prms[i])) == []


def test_depth_case_reaches_every_depth(cases, tables):
    (ctg,), sr, (prm,) = cases["depth"]
    depth = np.diff(ctg["col_off"]).tolist()
    assert depth == list(rc.DEPTHS) + [70, 70, 0]
    sel = lambda s: np.array([rc.selected(int(l), prm["which"]) for l in sr["labels"][ctg["col_idx"][ctg["col_off"][s]:ctg["col_off"][s + 1]]]], bool)
    assert sel(0).all() and sel(7).all() and not sel(8).any()      # the single entry is a row; a column of rows only; a column without any
    for s in range(1, 7):
        assert sel(s).any() and not sel(s).all()
    # the entry beyond the last full round of 64 of the deepest column is a row of its own or of an earlier entry: the tail round counts
    t = tables[("depth", 0)]
    flagged = np.unique(np.concatenate([ctg["col_idx"][ctg["col_off"][s]:ctg["col_off"][s + 1]][sel(s)] for s in range(9)]))
    assert np.array_equal(t["rows"]["read"], flagged) and len(flagged) > 1000
    assert int(t["rows"]["n_entries"].sum()) == sum(int(sel(s).sum()) for s in range(10))
    f = rc.forks(t, prm)
    assert f["absent"] > 100 and f["unclustered"] > 100 and f["assigned"] > 0 and f["empty_best"] > 0


def test_groups_case_reaches_both_decide_routes(cases, tables):
    ctgs, sr, (prm,) = cases["groups"]
    t = tables[("groups", 0)]
    at = rc.ac.rule_brute(ctgs, sr)
    assert np.diff(at["win_group_off"]).tolist() == list(rc.GROUP_SIZES)      # the window without a group is in the allele table ...
    assert np.diff(t["win_row_off"]).tolist() == [20, 20, 20, 20, 0, 20, 20]  # ... and has no rows
    assert sorted(set(t["row_groups"].tolist())) == [1, 2, 63, 64, 65, 300]
    f = rc.forks(t, prm)
    assert f["wide"] == 40 and f["lane"] == 80 and f["one_group"] == 20
    r, G = t["rows"], t["row_groups"]
    one = r[G == 1]
    assert (one["second_group"] == -1).all() and (one["m_second"] == 0).all() and (one["x_second"] == 0).all() and one["assigned"].any()      # margin vacuous
    for g in (2, 63, 64, 65, 300):
        rows = r[G == g]
        margin = (rows["m_best"].astype(int) - rows["x_best"]) - (rows["m_second"].astype(int) - rows["x_second"])
        assert (margin == 0).any() == (g > 8) and (rows["assigned"] != 0).any(), g       # ties (more groups than three SNPs tell apart) and unique bests
        tied = rows[margin == 0]
        assert (tied["assigned"] == 0).all() and (tied["best_group"] < tied["second_group"]).all()
    assert (r["best_group"] == 0).any() and (r["second_group"] == rc.ac.LARGE_ID).any() or (r["best_group"] == rc.ac.LARGE_ID).any()
    assert rc.ac.LARGE_ID in set(r["best_group"].tolist()) | set(r["second_group"].tolist()) and 0 in set(r["best_group"].tolist())


def test_which_case_selects_by_label(cases, tables):
    prms = cases["which"][2]
    f = [rc.forks(tables[("which", i)], prms[i]) for i in range(4)]
    assert (f[0]["absent"], f[0]["unclustered"], f[0]["labelled_own"] + f[0]["labelled_other"]) == (11, 0, 0)
    assert (f[1]["absent"], f[1]["unclustered"], f[1]["rows"]) == (0, 1, 1)
    assert (f[2]["absent"], f[2]["unclustered"], f[2]["labelled_own"], f[2]["labelled_other"]) == (0, 0, 12, 1)
    assert f[3]["rows"] == f[0]["rows"] + f[1]["rows"] + f[2]["rows"] == 25
    # a labelled row never changes a label, whatever its best group
    ctgs, sr, _ = cases["which"]
    t = tables[("which", 2)]
    assert t["rows"]["assigned"].all() and np.array_equal(rc.apply_numpy(t, sr), sr["labels"])


def test_rule_case_reaches_every_branch(cases, tables):
    prms = cases["rule"][2]
    f = [rc.forks(tables[("rule", i)], prms[i]) for i in range(4)]
    by_read = lambda i: {int(r["read"]): r for r in tables[("rule", i)]["rows"]}
    first = 10      # the extra reads follow the 2 x 5 core reads
    d, one = by_read(0), by_read(1)
    assert (f[0]["informative_below_min"] >= 1 and d[first + 0]["assigned"] == 0 and d[first + 0]["m_best"] == 2) and d[first + 1]["assigned"] == 1
    assert f[1]["margin_below_min"] == 1 and one[first + 2]["assigned"] == 0 and f[1]["margin_at_min"] == 2 and one[first + 3]["assigned"] == 1
    assert f[1]["tie_otherwise_fine"] == 1 and (one[first + 4]["best_group"], one[first + 4]["second_group"], one[first + 4]["assigned"]) == (0, 5, 0)
    assert f[0]["fraction_exact"] == 1 and d[first + 5]["assigned"] == 1 and (d[first + 5]["m_best"], d[first + 5]["x_best"]) == (3, 1)
    assert d[first + 6]["assigned"] == 0 and one[first + 6]["assigned"] == 1 and f[0]["fraction_alone_refuses"] == 2      # (reads 3 and 6)
    assert f[0]["negative_best"] == 1 and (d[first + 7]["best_group"], d[first + 7]["m_best"], d[first + 7]["x_best"], d[first + 7]["x_second"]) == (5, 0, 2, 3)
    assert f[0]["empty_best"] == 1 and (d[first + 8]["best_group"], d[first + 8]["m_best"], d[first + 8]["x_best"], d[first + 8]["n_entries"]) == (5, 0, 0, 1)
    assert d[first + 9]["m_best"] == 3 and d[first + 9]["assigned"] == 1      # THIRD matched the call of group 0
    assert (d[first + 10]["n_entries"], d[first + 10]["m_best"], d[first + 10]["assigned"]) == (3, 3, 1)      # twice in one column
    # 0/1: only rows without a mismatch; 1/1 and (2^31 - 1)/(2^31 - 1): the same table, the product needs 64 bits
    zero = tables[("rule", 2)]["rows"]
    assert ((zero["assigned"] != 0) <= (zero["x_best"] == 0)).all() and f[2]["assigned"] == 4
    assert rc.differences(tables[("rule", 1)], tables[("rule", 3)]) == [] and f[3]["assigned"] == 7


def test_windows_case_reaches_every_layout(cases, tables):
    ctgs, sr, (prm,) = cases["windows"]
    t = tables[("windows", 0)]
    assert t["win_contig"].tolist() == [0, 0, 0, 3, 4] and t["win_index"].tolist() == [0, 2, 3, 5, 6] and t["n_call_windows"] == 7
    assert len(ctgs[1]["snp_pos"]) == 0 and sr["win_off"][3] == sr["win_off"][2] and len(ctgs[3]["read_start"]) == 0
    reads0 = [set(t["rows"]["read"][t["win_row_off"][w]:t["win_row_off"][w + 1]].tolist()) for w in range(3)]
    assert reads0[0] & reads0[1] and reads0[1] & reads0[2]      # reads with rows in two windows of a contig
    c4 = ctgs[4]
    assert (c4["col_idx"] == -1).sum() == 4 and (c4["col_idx"] == len(c4["read_start"])).sum() == 4
    assert t["win_row_off"][3] == t["win_row_off"][4]      # the contig without reads: a window with a SNP and no rows
    last = t["rows"][t["win_row_off"][4]:]
    assert last["read"].tolist() == [0, 11] and last["n_entries"].tolist() == [4, 4] and last["best_group"].tolist() == [0, 1] and last["assigned"].tolist() == [1, 1]


def test_empty_case_gives_an_empty_table(tables):
    t = tables[("empty", 0)]
    assert len(t["rows"]) == 0 and len(t["win_start"]) == 0 and t["win_row_off"].tolist() == [0]


@pytest.mark.parametrize("wrong", rc.WRONG_RULES)
def test_a_bent_rule_gives_another_table(cases, tables, wrong):
    name, i = rc.WRONG_ON[wrong]
    ctgs, sr, prms = cases[name]
    assert rc.differences(tables[(name, i)], rc.recruit_brute(ctgs, sr, prms[i], wrong=wrong)) != []


def test_every_bent_rule_has_its_case():
    assert set(rc.WRONG_ON) == set(rc.WRONG_RULES) and len(rc.WRONG_RULES) == 10


@pytest.mark.parametrize("name,i", [("rule", 1), ("which", 3), ("windows", 0), ("groups", 0)])
def test_apply_in_numpy_is_the_selftests(built, cases, tables, tmp_path, name, i):
    ctgs, sr, prms = cases[name]
    exe = os.path.join(os.path.dirname(built["harness"]), "recruit_selftest")
    path = tmp_path / "call.json"
    path.write_text(rc.host_input(ctgs, sr, prms[i], len(ctgs) // 2))
    out = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, check=True).stdout.decode()
    labels = np.array(out.split("LABELS\n")[1].split("\n")[0].split(), np.int32)
    want = rc.apply_numpy(tables[(name, i)], sr)
    assert np.array_equal(labels, want)
    changed = np.flatnonzero(want != sr["labels"])
    assert len(changed) > 0 and (np.asarray(sr["labels"])[changed] < 0).all() and (want[changed] >= 0).all()
    assert len(changed) == int(((tables[(name, i)]["rows"]["assigned"] != 0) & (tables[(name, i)]["rows"]["label"] < 0)).sum())
