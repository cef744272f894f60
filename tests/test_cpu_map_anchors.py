"""The anchor rule without a device: the C++ host half (hs_map_host.cpp: map_anchors_host / map_anchors_of_keys, through tests/harness/map_anchor_selftest.cpp)
equals the numpy form of tests/anchor_cases.py on every case, field by field; every case reaches the fork it is named after (asserted from the chain's
members and the counters); each plausible wrong rule gives another result on the case that claims its fork; on noisy reads the alignment through the
anchors costs exactly what the HW optimum costs, by a DP that shares nothing with A1. tests/test_gpu_map_anchors.py holds the device to the same cases."""
import os
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import map_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")


@pytest.fixture(scope="module")
def exe(built):
    return built["map_anchor_selftest"]


def _same_hits(want, got):
    return got["returncode"] == 0 and all(int(got[f]) == int(want[f]) for f in ac.READ_FIELDS) and got["members"] == list(want["members"]) \
        and got["q"] == want["q"].tolist() and got["t"] == want["t"].tolist()


@pytest.mark.parametrize("name", sorted(ac.HIT_CASES))
def test_host_rule_equals_the_numpy_form_on_given_hits(exe, name):
    s, Lr, pairs = ac.HIT_CASES[name]
    got = ac.run_harness_hits(exe, s, Lr, pairs)
    assert _same_hits(ac.want_hits(name), got), (ac.want_hits(name), got)
    got = ac.run_harness_hits(exe, s, Lr, pairs[::-1])      # the order the hits come in does not matter
    assert _same_hits(ac.want_hits(name), got)


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_host_half_equals_the_numpy_form(exe, name):
    p, spacing, contigs, reads = ac.get(name)
    want = ac.want(name)
    got = ac.run_harness(exe, p, spacing, contigs, reads, threads=3)
    assert got["returncode"] == 0, got
    assert ac.differences(want, got) == []
    assert [f for f in mc.FIELDS if not np.array_equal(want["map"][f], got["map"][f])] == []
    assert ac.inside_interval(want["map"], want, reads)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_every_case_of_the_mapper(exe, name):
    """the mapper's fields are map_cases' own, unchanged; the anchors lie inside the interval, ascending strictly"""
    p, contigs, reads = mc.get(name)
    want = ac.want_map_case(name)
    got = ac.run_harness(exe, p, 64, contigs, reads)
    assert got["returncode"] == 0, got
    assert ac.differences(want, got) == []
    assert [f for f in mc.FIELDS if not np.array_equal(mc.want(name)[f], got["map"][f])] == []
    assert ac.inside_interval(got["map"], got, reads)
    mapped = mc.want(name)["contig"] >= 0
    assert (np.diff(want["anc_off"])[~mapped] == 0).all() and (want["n_best"][~mapped] == 0).all()


def test_host_half_under_sanitizers(built):
    """the same program built with -fsanitize=address,undefined, an executable of its own: hits at the capacity and above it, the lists given as they
    are, a chain that is not the whole list, no read at all"""
    subprocess.run(["make", "-s", "-f", "map_anchor_selftest.mk", "asan"], cwd=HARNESS, check=True)
    exe = os.path.join(HARNESS, "_build", "map_anchor_selftest_asan")
    for name in ("capacity", "lone_seed", "strands"):
        p, spacing, contigs, reads = ac.get(name)
        got = ac.run_harness(exe, p, spacing, contigs, reads, threads=2)
        assert got["returncode"] == 0, got
        assert ac.differences(ac.want(name), got) == []
    for name in sorted(ac.HIT_CASES):
        assert _same_hits(ac.want_hits(name), ac.run_harness_hits(exe, *ac.HIT_CASES[name]))
    assert ac.run_harness(exe, mc.params(), 256, [np.zeros(0, np.uint8)], [])["returncode"] == 0


def test_a_spacing_below_one_is_refused(exe):
    assert ac.run_harness(exe, mc.params(), 0, [np.zeros(30, np.uint8)], [])["returncode"] == 4
    assert ac.run_harness_hits(exe, 0, 100, [(1, 1)])["returncode"] == 4


# ---- every case reaches its fork ----
def _members(name):
    w = ac.want_hits(name)
    return [tuple(int(x) for x in w["hits"][i]) for i in w["members"]]


def test_fork_duplicates():
    assert _members("equal_qa") == [(10, 100), (20, 400), (30, 500), (40, 510)] and ac.want_hits("equal_qa")["n_best"] == 5
    assert _members("equal_t") == [(20, 100), (30, 200), (40, 210), (50, 220)]      # the later of the two replaced the earlier as the tail
    w = ac.want_hits("equal_t")
    assert w["n_supported"] == 3 and w["q"].tolist() == [30]      # (20, 100) is alone on its diagonal


def test_fork_canonical_chain():
    """two longest chains of equal length, (10, 100) .. and (20, 50) ..: the procedure's own wins, and a crossing pair stays out"""
    assert _members("two_longest") == [(20, 50), (30, 110), (40, 120)]
    m = _members("crossing")
    assert (35, 500) not in m and (36, 20) not in m and len(m) == 6 and ac.want_hits("crossing")["n_best"] == 8
    assert _members("descending") == [(30, 70)] and ac.want_hits("descending")["n_supported"] == 0 and len(ac.want_hits("descending")["q"]) == 0
    assert ac.want_hits("one_hit")["n_chain"] == 1 and len(ac.want_hits("one_hit")["q"]) == 0      # a lone hit has no neighbour: no anchor


def test_fork_support():
    w = ac.want_hits("lone_diagonal")
    s = ac.HIT_CASES["lone_diagonal"][0]
    assert (w["n_chain"], w["n_supported"]) == (5, 4) and (110, 205) in _members("lone_diagonal")
    assert 110 - 10 >= s and w["q"].tolist() == [10, 150]      # the lone member lies a spacing behind the first cut and is passed over


def test_fork_spacing():
    s = ac.HIT_CASES["spacing_edge"][0]
    assert ac.want_hits("spacing_edge")["q"].tolist() == [0, s, 2 * s]      # s - 1 behind a cut: none; s: one
    assert ac.want_hits("from_last_cut")["q"].tolist() == [0, 120]
    w = ac.want_hits("spacing_one")
    sup = [i for j, i in enumerate(w["members"]) if j in _supported_positions(w)]
    assert ac.HIT_CASES["spacing_one"][0] == 1 and w["q"].tolist() == [int(w["hits"][i][0]) for i in sup] and w["n_supported"] == len(w["q"]) >= 8


def _supported_positions(w):
    d = [int(w["hits"][i][1] - w["hits"][i][0]) for i in w["members"]]
    return {j for j in range(len(d)) if (j > 0 and d[j - 1] == d[j]) or (j + 1 < len(d) and d[j + 1] == d[j])}


def test_fork_strands_unmapped_capacity():
    p, spacing, contigs, reads = ac.get("strands")
    w = ac.want("strands")
    assert w["map"]["strand"].tolist() == [1, 0] and np.diff(w["anc_off"]).tolist() == [np.diff(w["anc_off"])[0]] * 2 and w["anc_off"][1] >= 5
    half = int(w["anc_off"][1])
    assert np.array_equal(w["anc_q"][:half] + 700, w["anc_t"][:half])      # an error-free read: every anchor on the true diagonal
    # the reverse complement's hits are the same k-mers: qa = Lr - k - q puts them on the same diagonal of the read as it aligns
    assert np.array_equal(w["anc_q"][half:] + 700, w["anc_t"][half:])
    w = ac.want("unmapped")
    assert w["map"]["contig"].tolist() == [-1, -1, 0] and np.diff(w["anc_off"])[:2].tolist() == [0, 0] and w["n_best"][:2].tolist() == [0, 0]
    w = ac.want("capacity")
    assert w["map"]["n_hits"].tolist() == [mc.LDS_CAPACITY, mc.LDS_CAPACITY + 1] and (w["map"]["contig"] >= 0).all()
    assert w["n_best"][0] > 0 and w["n_chain"][0] > 0 and [w["n_best"][1], w["n_chain"][1], w["n_supported"][1]] == [0, 0, 0] and w["anc_off"][1] == w["anc_off"][2]


@pytest.mark.parametrize("wrong,name", [("non_strict", "equal_t"), ("both_ascending", "equal_qa"), ("upper_bound", "equal_t"), ("no_support", "lone_diagonal"),
                                        ("from_previous", "from_last_cut")])
def test_a_wrong_rule_gives_another_result(wrong, name):
    s, Lr, pairs = ac.HIT_CASES[name]
    a, b = ac.want_hits(name), ac.anchors_of_hits([x[0] for x in pairs], [x[1] for x in pairs], Lr, s, wrong=wrong)
    assert wrong in ac.WRONG
    assert (a["n_chain"], a["n_supported"], a["q"].tolist(), a["t"].tolist()) != (b["n_chain"], b["n_supported"], b["q"].tolist(), b["t"].tolist())


def test_without_the_support_rule_a_lone_seed_costs_edits():
    """lone_seed: the chain holds a seed on a foreign diagonal between two runs. The rule passes it over and the alignment through the anchors costs what the
    HW optimum costs; with every member trusted the cut through it costs more, by the DP of anchor_cases"""
    p, spacing, contigs, reads = ac.get("lone_seed")
    w = ac.want("lone_seed")
    b = ac.anchors_numpy(p, spacing, contigs, reads, wrong="no_support", res=w["map"])
    m = w["map"]
    iv = (0, 0, m["strand"][0], m["qstart"][0], m["qend"][0], m["tstart"][0], m["tend"][0])
    nm_rule, nm_hw = ac.anchored_distance(reads[0], contigs[0], iv, w["anc_q"], w["anc_t"])
    nm_wrong, _ = ac.anchored_distance(reads[0], contigs[0], iv, b["anc_q"], b["anc_t"])
    assert len(set((w["anc_t"] - w["anc_q"]).tolist())) == 1 and len(set((b["anc_t"] - b["anc_q"]).tolist())) > 1
    assert nm_rule == nm_hw and nm_wrong > nm_hw, (nm_rule, nm_wrong, nm_hw)


# ---- noisy reads ----
@pytest.mark.parametrize("spacing", [128, 256, 512])
def test_every_noisy_read_has_a_cut_point(exe, spacing):
    c, p, contigs, want = ac.noisy(spacing)
    got = ac.run_harness(exe, p, spacing, contigs, c.reads, threads=4)
    assert got["returncode"] == 0, got
    assert ac.differences(want, got) == [] and ac.inside_interval(got["map"], got, c.reads)
    assert len(c.reads) == 310 and (want["map"]["contig"] >= 0).all() and (np.diff(want["anc_off"]) >= 1).all()
    for r in range(len(c.reads)):      # no piece between two cut points shorter than the spacing
        assert (np.diff(want["anc_q"][want["anc_off"][r]:want["anc_off"][r + 1]]) >= spacing).all()


def test_noisy_anchored_distance_is_the_optimum():
    """the first 40 reads at spacing 256: NM through the anchors == NM of the HW optimum in the same window, read by read (an integer condition the rule
    meets on this case; all 310 at 128, 256 and 512 were run once by hand and hold too). NM(anchored) >= NM(plain) holds by construction."""
    c, p, contigs, want = ac.noisy(256)
    m = want["map"]
    for r in range(40):
        iv = (r, 0, m["strand"][r], m["qstart"][r], m["qend"][r], m["tstart"][r], m["tend"][r])
        a, b = int(want["anc_off"][r]), int(want["anc_off"][r + 1])
        nm, hw = ac.anchored_distance(c.reads[r], c.seq, iv, want["anc_q"][a:b], want["anc_t"][a:b])
        assert nm == hw, (r, nm, hw)
