"""The split mapper's rule without a device: the C++ host half (hs_map_host.cpp: map_reads_split_host, through tests/harness/map_split_selftest.cpp) equals the
numpy form of tests/map_split_cases.py on every case, field by field, and its text the restated PAF; every case reaches the fork it is named after (asserted
from the rounds, gaps and free counts the numpy form exposes); each plausible wrong rule gives another result on the case that claims its fork; error-free
reads over a cut come back as exactly their parts. tests/test_gpu_map_split.py holds the device to the same cases."""
import os
import subprocess

import numpy as np
import pytest

import map_cases as mc
import map_split_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")
NAMES = sorted(sc.CASES)


@pytest.fixture(scope="module")
def exe(built):
    return built["map_split_selftest"]


@pytest.mark.parametrize("name", NAMES)
def test_host_half_equals_the_numpy_form(exe, name):
    p, sp, contigs, reads = sc.get(name)
    want = sc.want(name)
    got = sc.run_harness(exe, p, sp, contigs, reads, threads=3)
    assert got["returncode"] == 0, got
    assert sc.differences(want, got) == []
    assert got["text"] == sc.paf(want, contigs, reads)


def test_host_half_under_sanitizers(built):
    """the same program built with -fsanitize=address,undefined, an executable of its own: eight segments of one read, the scratch-route sizes, no read at all"""
    subprocess.run(["make", "-s", "-f", "map_split_selftest.mk", "asan"], cwd=HARNESS, check=True)
    exe = os.path.join(HARNESS, "_build", "map_split_selftest_asan")
    for name in ("nine_parts", "wide", "enclose"):
        p, sp, contigs, reads = sc.get(name)
        got = sc.run_harness(exe, p, sp, contigs, reads, threads=2)
        assert got["returncode"] == 0, got
        assert sc.differences(sc.want(name), got) == []
    assert sc.run_harness(exe, sc.params(), sc.split(), [np.zeros(0, np.uint8)], [])["returncode"] == 0


@pytest.mark.parametrize("bad", [dict(max_segments=0), dict(max_segments=9), dict(min_votes=0), dict(min_span=-1), dict(max_gap=-1)])
def test_parameters_out_of_range_are_refused(exe, bad):
    assert not sc.split_valid(sc.split(**bad))
    assert sc.run_harness(exe, sc.params(), sc.split(**bad), [np.zeros(30, np.uint8)], [])["returncode"] == 4


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_one_segment_is_the_plain_mapper(exe, name):
    """max_segments = 1 on every case of map_cases: every field of map_cases.FIELDS as the plain rule's numpy form has it, from the numpy form and from the host half"""
    p, contigs, reads = mc.get(name)
    sp = sc.split(max_segments=1)
    got = sc.run_harness(exe, p, sp, contigs, reads)
    assert got["returncode"] == 0, got
    for res in (sc.split_numpy(p, sp, contigs, reads), got):
        one = sc.as_map_result(res)
        assert [f for f in mc.FIELDS if not np.array_equal(one[f], mc.want(name)[f])] == []
        assert (res["round"] == 0).all()


# ---- truth ----
def test_error_free_reads_over_a_cut_come_back_as_exactly_their_parts(exe):
    """no tolerance: a read window inside a piece is a window of that piece, so every hit lies on the true diagonal; the gap at a cut is below k + w, and the
    clip at the contig's end puts the boundary on the cut. The segments of a read are its parts (each of 300 bases or more), all of them and nothing else."""
    p, sp, contigs, reads = sc.get("junction_exact")
    truth = sc.junction_truth()
    host = sc.run_harness(exe, p, sp, contigs, reads)
    assert host["returncode"] == 0, host
    assert len(reads) >= 40 and all(700 <= len(r) <= 4000 for r in reads)
    n_parts = [len([x for x in parts if x[4] - x[3] >= 300]) for parts in truth]
    assert sum(n == 2 for n in n_parts[:12]) == 12 and n_parts[12:14] == [3, 3]
    assert {parts[0][2] for parts in truth[:14]} == {0, 1}      # both strands among the constructed reads
    for res in (host, sc.want("junction_exact")):      # the host half and the numpy form, each against the truth
        for r, parts in enumerate(truth):
            assert sc.rows(res, r) == parts, (r, parts, sc.rows(res, r))
        for r in (12, 13):      # over 20 000 and 21 000: the middle segment is the whole 1 000-base piece
            mid = sc.rows(res, r)[1]
            assert mid[1] == 2 and (mid[5], mid[6]) == (0, 1000) and mid[4] - mid[3] == 1000
        assert (res["n_hits"] > 0).all() and (np.diff(res["seg_off"]) >= 1).all()


def test_noisy_reads_over_a_cut(exe):
    """test_cpu_map_cases.noisy_case() with its contig cut at 5 000, default parameters: a read with 500 true bases or more on both pieces has exactly two
    segments, on the two pieces and the true strand; a read that lies in one piece has no second segment; every segment's window, 100 bases wider on either
    side, holds the read's true span on its piece. Held on the host half's result, which equals the numpy form's on every field and in its text. The counts
    are the seed's: 310 reads, none without a segment, 35 with 500 bases or more on both pieces, 234 inside one piece."""
    from hairsplitter_amd import synth
    c, p, sp, contigs = sc.noisy()
    want = sc.split_numpy(p, sp, contigs, c.reads)
    res = sc.run_harness(exe, p, sp, contigs, c.reads, threads=3)
    assert res["returncode"] == 0, res
    assert sc.differences(want, res) == [] and res["text"] == sc.paf(want, contigs, c.reads)
    n_both = n_one = 0
    for a in c.alns:
        ops, lens = a.cigar & 0xF, a.cigar >> 4
        end = a.pos + int(lens[(ops == synth.OP_M) | (ops == synth.OP_D) | (ops == synth.OP_EQ) | (ops == synth.OP_X)].sum())
        true = {0: (a.pos, min(end, sc.NOISY_CUT)), 1: (max(a.pos, sc.NOISY_CUT) - sc.NOISY_CUT, end - sc.NOISY_CUT)}
        true = {k: v for k, v in true.items() if v[1] > v[0]}
        segs = sc.rows(res, a.read)
        if len(true) == 2 and min(v[1] - v[0] for v in true.values()) >= 500:
            n_both += 1
            assert sorted(s[1] for s in segs) == [0, 1] and all(bool(s[2]) == a.strand for s in segs), (a.read, segs)
        if len(true) == 1:
            n_one += 1
            assert len(segs) <= 1, (a.read, segs)
        for s in segs:
            assert s[1] in true and bool(s[2]) == a.strand and s[5] - 100 <= true[s[1]][0] and true[s[1]][1] <= s[6] + 100, (a.read, s, true)
    assert (len(c.alns), int((np.diff(res["seg_off"]) == 0).sum()), n_both, n_one) == (310, 0, 35, 234)


# ---- every case reaches its fork ----
def _rounds(name, r=0):
    return sc.want(name)["detail"][r]


def test_fork_same_key_in_two_gaps():
    """enclose: round 0 takes the middle part; rounds 1 and 2 take the SAME key on the other contig, one gap each, the fuller gap first"""
    for r in (0, 1):
        d = _rounds("enclose", r)
        assert [x["taken"] for x in d] == [True, True, True, False] and d[3]["n_free"] == 0
        assert d[0]["best"][0] == 1 and d[1]["best"] == d[2]["best"] and d[1]["best"][0] == 0
        assert min(d[1]["gap_counts"]) > 0 and d[1]["n"] == max(d[1]["gap_counts"]) and d[1]["score"] == sum(d[1]["gap_counts"])
        assert d[2]["n"] == min(d[1]["gap_counts"]) and d[2]["gap"] != d[1]["gap"]
        assert d[1]["n_free"] == d[0]["n_free"] - d[0]["n"] and d[2]["n_free"] == d[1]["n_free"] - d[1]["n"]
    res = sc.want("enclose")
    assert res["contig"].tolist() == [0, 1, 0, 0, 1, 0] and res["round"][[1, 4]].tolist() == [0, 0]
    d = _rounds("gap_tie")
    assert d[1]["gap_counts"][0] == d[1]["gap_counts"][1] > 0 and d[1]["gap"] == 0      # the leftmost gap on a tie


def test_fork_free_hits():
    """shared: round 0's span ends inside a stretch that both contigs hold; some hit of round 1's key starts one base before that end (not free), and no hit
    that overlaps the span is counted"""
    p, sp, contigs, reads = sc.get("shared")
    H = sc.hits_numpy(p, mc.index_numpy(p, contigs), reads[0])
    d = _rounds("shared")
    a0, a1 = d[0]["span"]
    other = (H["c"] == d[1]["best"][0]) & (H["rel"] == d[1]["best"][1])
    overlap = other & ~((H["q"] + p["k"] <= a0) | (H["q"] >= a1))
    assert overlap.any() and (((H["q"] + p["k"] == a0 + 1) | (H["q"] == a1 - 1)) & other).any()
    assert d[1]["n_free"] == int(((H["q"] + p["k"] <= a0) | (H["q"] >= a1)).sum())
    assert d[1]["n"] == int((other & ~overlap & ((H["b"] == d[1]["best"][2]) | (H["b"] == d[1]["best"][2] + 1))).sum())


def test_fork_max_gap():
    p, sp, contigs, reads = sc.get("insert")
    res = sc.want("insert")
    # read 0: 1500 foreign bases: the inner ends stay at the seed bounds, the outer ends reach the read's ends
    d = sorted(x["span"] for x in _rounds("insert", 0) if x["taken"])
    r = sc.rows(res, 0)
    assert d[1][0] - d[0][1] > sp["max_gap"] and (r[0][3], r[0][4], r[1][3], r[1][4]) == (0, d[0][1], d[1][0], len(reads[0]))
    # reads 1 and 2: exactly max_gap | max_gap + 1 between the spans: both sides extended | neither
    gaps = []
    for i in (1, 2):
        d = sorted(x["span"] for x in _rounds("insert", i) if x["taken"])
        gaps.append(d[1][0] - d[0][1])
        r = sc.rows(res, i)
        assert (r[0][4], r[1][3]) == ((d[1][0], d[0][1]) if i == 1 else (d[0][1], d[1][0]))
    assert gaps == [sp["max_gap"], sp["max_gap"] + 1]


def test_fork_limits():
    res = sc.want("three_parts")
    assert sc.get("three_parts")[1]["max_segments"] == 2 and res["contig"].tolist() == [0, 1] and len(_rounds("three_parts")) == 2
    res = sc.want("nine_parts")      # eight of nine: the ninth part is left out, and its neighbour is not stretched over it
    assert np.diff(res["seg_off"]).tolist() == [8, 8] and sorted(res["round"][:8].tolist()) == list(range(8))
    for r in (0, 1):
        rows = sc.rows(res, r)
        assert len({x[1] for x in rows}) == 8 and all((x[5], x[6], x[4] - x[3]) == (0, 400, 400) for x in rows)
    sp = sc.get("min_span")[1]
    d0, d1 = _rounds("min_span", 0), _rounds("min_span", 1)
    assert [d0[1]["span"][1] - d0[1]["span"][0], d1[1]["span"][1] - d1[1]["span"][0]] == [sp["min_span"] - 1, sp["min_span"]]
    assert d0[1]["n"] >= sp["min_votes"] and not d0[1]["taken"] and d1[1]["taken"] and np.diff(sc.want("min_span")["seg_off"]).tolist() == [1, 2]
    p, sp = sc.get("min_votes")[:2]
    d0, d1 = _rounds("min_votes", 0), _rounds("min_votes", 1)
    assert sp["min_votes"] > p["min_votes"] and [d0[1]["score"], d1[1]["score"]] == [sp["min_votes"] - 1, sp["min_votes"]]
    assert not d0[1]["taken"] and d1[1]["taken"] and np.diff(sc.want("min_votes")["seg_off"]).tolist() == [1, 2]


def test_fork_stop():
    """round 1's best candidate fails min_span in the gap it keeps; the part on the third contig would stand, and is not tried"""
    p, sp, contigs, reads = sc.get("stop")
    d = _rounds("stop")
    assert len(d) == 2 and not d[1]["taken"] and d[1]["best"][0] == 0 and d[1]["n"] >= sp["min_votes"] and d[1]["span"][1] - d[1]["span"][0] < sp["min_span"]
    assert d[1]["score"] == sum(d[1]["gap_counts"]) > d[1]["n"]
    skip = sc.split_numpy(p, sp, contigs, reads, wrong="skip")
    assert 2 in skip["contig"].tolist() and sc.want("stop")["contig"].tolist() == [1]


def test_fork_capacity():
    assert (sc.want("wide")["n_hits"] > mc.LDS_CAPACITY).all() and sc.n_wide(sc.want("wide")) == 2
    assert sc.want("capacity")["n_hits"].tolist() == [mc.LDS_CAPACITY] and sc.n_wide(sc.want("capacity")) == 0
    for name in ("wide", "capacity"):      # the part on the other contig is a second segment on either route
        res = sc.want(name)
        assert (np.diff(res["seg_off"]) == 2).all() and set(res["contig"].tolist()) == {0, 1} and sorted(res["round"][:2].tolist()) == [0, 1]


@pytest.mark.parametrize("wrong,name", [("overlap_one", "shared"), ("no_gap", "enclose"), ("rightmost_gap", "gap_tie"), ("always_extend", "insert"), ("skip", "stop"),
                                        ("index_min_votes", "min_votes")])
def test_a_wrong_rule_gives_another_result(wrong, name):
    p, sp, contigs, reads = sc.get(name)
    assert wrong in sc.WRONG and not sc.same(sc.want(name), sc.split_numpy(p, sp, contigs, reads, wrong=wrong))
