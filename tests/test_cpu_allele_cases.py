"""tests/allele_cases.py without a device: the two statements of the rule agree on every case, every case reaches the fork it is there for (asserted on
counts derived from the case itself), and a rule bent in one place gives another table on the case aimed at that place."""
import numpy as np
import pytest

import allele_cases as ac

LDS_CAP = 2048      # (any capacity does here: the device tests take the library's own)


@pytest.fixture(scope="module")
def cases():
    return {name: ac.get(name, LDS_CAP) for name in ac.CASES}


@pytest.fixture(scope="module")
def tables(cases):
    return {name: ac.rule_brute(*cases[name]) for name in cases}


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_the_two_forms_agree(cases, tables, name):
    assert ac.differences(tables[name], ac.rule_numpy(*cases[name])) == []


def _cells(t, s):
    return t["cells"][int(t["snp_cell_off"][s]):int(t["snp_cell_off"][s + 1])]


def test_depths_case_reaches_every_depth(cases, tables):
    (ctg,), sr = cases["depths"]
    depth = np.diff(ctg["col_off"]).tolist()
    assert depth == [1, 63, 64, 65, 255, 256, LDS_CAP, LDS_CAP + 1]
    t = tables["depths"]
    assert t["group_ids"].tolist() == [0, 3, 7] and len(t["snp_pos"]) == len(depth)
    for s, d in enumerate(depth):
        lab = sr["labels"][ctg["col_idx"][ctg["col_off"][s]:ctg["col_off"][s + 1]]]
        assert int(_cells(t, s)["n"].sum()) == int((lab >= 0).sum())
        if d >= 63:
            assert (lab == -1).any() and (lab == -2).any() and (lab >= 0).any()


def test_groups_case_reaches_every_group_count(cases, tables):
    _, sr = cases["groups"]
    t = tables["groups"]
    counts = np.diff(t["win_group_off"]).tolist()
    assert counts == [1, 2, 63, 64, 0, 65, 300]
    assert ac.LARGE_ID in t["group_ids"].tolist() and 6 in t["group_ids"].tolist() and 1 not in t["group_ids"].tolist()
    for w in range(len(counts)):
        ids = t["group_ids"][t["win_group_off"][w]:t["win_group_off"][w + 1]]
        assert np.all(np.diff(ids.astype(np.int64)) > 0)
    w = counts.index(0)
    assert np.all(sr["labels"][sr["label_off"][w]:sr["label_off"][w + 1]] < 0) and t["win_snp_off"][w + 1] - t["win_snp_off"][w] == 2
    # every second group has no entry on the window's second SNP
    s = int(t["win_snp_off"][counts.index(300)]) + 1
    assert (_cells(t, s)["n"] == 0).any() and (_cells(t, s)["n"] > 0).any()


def test_codes_case_reaches_every_branch(tables):
    t = tables["codes"]
    names = list(ac.CODE_SCENARIOS)
    cell = lambda name, g: _cells(t, names.index(name))[g]
    assert t["group_ids"].tolist() == [0, 1]
    x = cell("tie_top", 0)
    assert (x["best"], x["second"], x["best_code"], x["call"], x["n"]) == (5, 5, 40, 0, 10)
    x = cell("tie_second", 0)
    assert (x["best"], x["second"], x["call"]) == (10, 2, 40)
    x = cell("second_half_of_best", 0)
    assert 2 * x["second"] == x["best"] and x["call"] == 40
    x = cell("second_half_of_best", 1)
    assert 2 * x["second"] == x["best"] and x["call"] == 47 and x["n_ref"] == 6
    x = cell("second_above_half", 0)
    assert 2 * x["second"] == x["best"] + 1 and x["call"] == 0 and x["n"] <= 2 * x["best"]
    x = cell("n_twice_best", 0)
    assert x["n"] == 2 * x["best"] and 2 * x["second"] <= x["best"] and x["call"] == 40
    x = cell("n_above_twice_best", 0)
    assert x["n"] == 2 * x["best"] + 1 and 2 * x["second"] <= x["best"] and x["call"] == 0
    assert len(ac.CODE_SCENARIOS["five_codes"][0]) > 4 and cell("five_codes", 0)["call"] == 40
    assert len(ac.CODE_SCENARIOS["all_codes"][0]) == 125 == len(ac.CODES)
    x = cell("all_codes", 0)
    assert (x["n"], x["best"], x["second"], x["best_code"], x["call"]) == (126, 2, 1, 33, 0)
    assert cell("ref_absent", 0)["n_ref"] == 0 and cell("ref_absent", 0)["call"] == 47
    assert cell("alt_absent", 0)["n_alt"] == 0 and cell("alt_absent", 1)["n_alt"] == 0
    x = cell("group_absent", 0)
    assert tuple(int(v) for v in x) == (0, 0, 0, 0, 0, 0, 0)
    s = names.index("second_half_of_best")
    assert t["snp_n_calls"][s] == 2 and t["snp_n_calls"][names.index("tie_top")] == 1 and t["snp_n_calls"][names.index("alt_absent")] == 1


def test_labels_case_has_entries_that_must_not_count(cases, tables):
    (ctg,), sr = cases["labels"]
    t = tables["labels"]
    assert np.diff(t["win_group_off"]).tolist() == [2, 3]
    lab_a = sr["labels"][:sr["label_off"][1]]
    in_col = lab_a[ctg["col_idx"][:ctg["col_off"][1]]]
    assert (in_col == -1).sum() == 9 and (in_col == -2).sum() == 9
    assert int(_cells(t, 0)["n"].sum()) == 12 and int(_cells(t, 1)["n"].sum()) == 21
    assert _cells(t, 0)["call"].tolist() == [40, 47] and _cells(t, 1)["call"].tolist() == [40, 47, 52]


def test_windows_case_layout(cases, tables):
    ctgs, sr = cases["windows"]
    t = tables["windows"]
    assert ctgs[0]["col_off"][0] == 7
    assert list(zip(t["win_contig"].tolist(), t["win_start"].tolist(), t["win_end"].tolist())) == [(0, 0, 499), (0, 1000, 1499), (0, 1500, 3600), (3, 0, 799)]
    assert np.diff(t["win_snp_off"]).tolist() == [2, 2, 1, 1]
    assert t["snp_pos"].tolist() == [0, 499, 1000, 1001, 2600, 300] and t["snp_contig"].tolist() == [0] * 5 + [3]
    assert 3650 in ctgs[0]["snp_pos"].tolist() and len(ctgs[1]["snp_pos"]) == 0 and sr["win_off"][3] - sr["win_off"][2] == 0 and len(ctgs[2]["snp_pos"]) == 1
    assert sr["win_end"][3] - sr["win_start"][3] > 2 * (sr["win_end"][0] - sr["win_start"][0])


def test_deepest_case_reaches_the_deepest_column(cases, tables):
    (ctg,), _ = cases["deepest"]
    depth = np.diff(ctg["col_off"])
    assert depth[0] == 65535 and depth.max() == 65535 and (depth[1:] == LDS_CAP + 1).all() and len(depth) - 1 == ac.WIDE_COLUMNS > 64
    t = tables["deepest"]
    assert t["group_ids"].tolist() == [2, 5, 6] and int(_cells(t, 0)["n"].sum()) < 65535 and (_cells(t, 0)["n"] > 16000).all()
    assert (t["snp_n_calls"][1:] == 2).all()


def test_empty_case(tables):
    t = tables["empty"]
    assert len(t["win_start"]) == 0 and len(t["cells"]) == 0 and t["snp_cell_off"].tolist() == [0]


@pytest.mark.parametrize("wrong,name,key", [("second_ge", "codes", "cells"), ("n_ge", "codes", "cells"), ("tie_largest", "codes", "cells"),
                                            ("minus1_group", "labels", "group_ids"), ("pos_lt_end", "windows", "snp_pos"), ("second_distinct", "codes", "cells")])
def test_a_wrong_rule_gives_another_table(cases, tables, wrong, name, key):
    assert wrong in ac.WRONG_RULES
    assert key in ac.differences(tables[name], ac.rule_brute(*cases[name], wrong=wrong))


def test_each_wrong_rule_is_caught_by_the_scenario_aimed_at_it(cases, tables):
    t = tables["codes"]
    names = list(ac.CODE_SCENARIOS)
    aimed = {"second_ge": "second_half_of_best", "n_ge": "n_twice_best", "tie_largest": "tie_top", "second_distinct": "tie_top"}
    for wrong, scenario in aimed.items():
        u = ac.rule_brute(*cases["codes"], wrong=wrong)
        s = names.index(scenario)
        assert _cells(t, s).tolist() != _cells(u, s).tolist(), wrong
