"""The read mapper's rule without a device: the C++ host half (hs_map_host.cpp through tests/harness/map_selftest.cpp) equals the numpy form of
tests/map_cases.py on every case, field by field; every case reaches the fork it is named after (asserted from the numpy form's counters); and each
plausible wrong rule gives another result on the case that claims its fork. tests/test_gpu_map.py holds the device to the same cases."""
import os
import subprocess

import numpy as np
import pytest

import map_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")
NAMES = sorted(mc.CASES)


@pytest.fixture(scope="module")
def exe(built):
    return os.path.join(HARNESS, "_build", "map_selftest")


@pytest.mark.parametrize("name", NAMES)
def test_host_half_equals_the_numpy_form(exe, name):
    p, contigs, reads = mc.get(name)
    want = mc.want(name)
    got = mc.run_harness(exe, p, contigs, reads, threads=3)
    assert got["returncode"] == 0, got
    assert mc.differences(want, got) == []
    assert got["text"] == mc.paf(want, contigs, reads)


def test_host_half_under_sanitizers(built):
    """the same program built with -fsanitize=address,undefined, an executable of its own: the length edges and the scratch-route sizes"""
    subprocess.run(["make", "-s", "-f", "map_selftest.mk", "asan"], cwd=HARNESS, check=True)
    for name in ("lengths", "no_contigs", "capacity"):
        p, contigs, reads = mc.get(name)
        got = mc.run_harness(os.path.join(HARNESS, "_build", "map_selftest_asan"), p, contigs, reads, threads=2)
        assert got["returncode"] == 0, got
        assert mc.differences(mc.want(name), got) == []


@pytest.mark.parametrize("bad", [dict(k=4), dict(k=17), dict(w=0), dict(w=33), dict(max_occ=0), dict(band_log2=31), dict(min_votes=0), dict(extend=2), dict(bucket_bits=27)])
def test_parameters_out_of_range_are_refused(exe, bad):
    assert mc.run_harness(exe, mc.params(**bad), [np.zeros(30, np.uint8)], [])["returncode"] == 4


# ---- every case reaches its fork ----
def test_fork_lengths():
    p, contigs, reads = mc.get("lengths")
    w = mc.want("lengths")
    assert [len(r) for r in reads[:5]] == [0, p["k"] - 1, p["k"], p["k"] + p["w"] - 2, p["k"] + p["w"] - 1]
    assert w["n_minimizers"][:5].tolist() == [0, 0, 1, 1, 1]      # below k bases none; up to k + w - 1 bases one window of all the k-mers
    # (a shorter read's only minimizer need not be one of the contig's: from k + w - 1 bases on a read window is a contig window)
    assert w["contig"][:2].tolist() == [-1, -1] and (w["contig"][4], w["tstart"][4], w["tend"][4]) == (0, 400, 400 + p["k"] + p["w"] - 1)
    assert set(w["index"]["c"].tolist()) == {0}      # the contig shorter than k and the empty one have no entry
    assert len(mc.want("no_reads")["contig"]) == 0
    for name in ("no_contig_minimizers", "no_contigs"):
        assert len(mc.want(name)["index"]["h"]) == 0 and mc.want(name)["n_hits"].sum() == 0 and (mc.want(name)["contig"] == -1).all()


@pytest.mark.parametrize("k,w", [(5, 1), (5, 32), (15, 10), (16, 1), (16, 32)])
def test_fork_params(k, w):
    name = "k%d_w%d" % (k, w)
    p, contigs, reads = mc.get(name)
    res = mc.want(name)
    assert (p["k"], p["w"]) == (k, w)
    if w == 1:      # every k-mer that is not skipped is a minimizer
        assert res["n_minimizers"][4] == mc.kmers(reads[4], k)[2].sum()
    if k == 5:
        assert (res["n_hits"] > 4 * res["n_minimizers"]).all() and len(set(res["index"]["h"].tolist())) <= 512      # 4^5 / 2 words over 4500 bases: every hash many times
    else:
        assert res["contig"][:4].tolist() == [0, 0, 1, 1] and res["strand"][:4].tolist() == [1, 0, 1, 0] and res["tstart"][:4].tolist() == [100, 1000, 50, 1100]
        assert res["contig"][4] == -1
    if k == 16:      # all 32 bits of the word in use: minimizers whose k-mer has the top bit of its forward word set (first base G or T)
        pos = res["minimizers"][0][0]
        assert (reads[0][pos] >= 2).any() and (w > 1 or (res["minimizers"][0][1] >= 1 << 31).any())


def test_fork_ties():
    res = mc.want("homopolymer")
    p = mc.get("homopolymer")[0]
    assert res["n_minimizers"][2] == 60 - p["k"] + 1 - p["w"] + 1      # inside the run every window names its leftmost k-mer: one per window
    assert len(set(res["minimizers"][2][1].tolist())) == 1
    res = mc.want("palindromes")
    p, contigs, reads = mc.get("palindromes")
    assert len(reads[1]) >= p["k"] + p["w"] - 1 and res["n_minimizers"][1] == 0 and not mc.kmers(reads[1], p["k"])[2].any()


def test_fork_occ():
    res = mc.want("occ")
    assert 64 in res["detail"][0]["occ_used"].tolist() and len(res["detail"][0]["occ_skipped"]) == 0 and res["n_hits"][0] >= 64
    assert 65 in res["detail"][1]["occ_skipped"].tolist() and res["n_skipped"][1] >= 1


def test_fork_bins():
    res = mc.want("bins")
    d = res["detail"]
    assert d[0]["best"][2] == 1 and d[1]["best"][2] == 2 and len(d[0]["bins"]) == 1 and len(d[1]["bins"]) == 1
    b = d[2]["best"][2]
    assert d[2]["bins"].get(b, 0) > 0 and d[2]["bins"].get(b + 1, 0) > 0 and res["votes"][2] == d[2]["bins"][b] + d[2]["bins"][b + 1] == res["n_hits"][2]
    bins = sorted(d[3]["bins"])
    assert bins[-1] - bins[0] == 3 and res["votes"][3] < res["n_hits"][3] and res["second"][3] > 0


def test_fork_order():
    res = mc.want("identical_contigs")
    assert res["contig"].tolist() == [0, 0] and (res["second"] == res["votes"]).all()
    res = mc.want("self_rc")
    assert res["strand"][0] == 1 and res["second"][0] == res["votes"][0] and res["detail"][0]["best"][1] == 0


def test_fork_ends():
    p, contigs, reads = mc.get("ends_extend1")
    res = mc.want("ends_extend1")
    i = 0
    for h in (1, 200):
        for k, (q, t) in enumerate([((h, 500), (0, 500 - h)), ((0, 500 - h), (2500 + h, 3000))]):
            for minus in (0, 1):
                r = i + k + 2 * minus
                assert (res["contig"][r], res["strand"][r], res["tstart"][r], res["tend"][r]) == (0, 1 - minus, t[0], t[1])
                assert (res["qstart"][r], res["qend"][r]) == (q if not minus else (500 - q[1], 500 - q[0]))
        i += 4
    for r in (8, 9):      # the read longer than its contig
        assert (res["contig"][r], res["qstart"][r], res["qend"][r], res["tstart"][r], res["tend"][r]) == (1, 100, 500, 0, 400)
    seeds = mc.want("ends_extend0")
    assert (seeds["tstart"] >= res["tstart"]).all() and (seeds["tend"] <= res["tend"]).all() and (seeds["tend"] - seeds["tstart"] < res["tend"] - res["tstart"]).any()
    assert np.array_equal(seeds["qend"] - seeds["qstart"], seeds["tend"] - seeds["tstart"])


def test_fork_capacity():
    assert (mc.want("tandem")["n_hits"] > mc.LDS_CAPACITY).all() and mc.n_wide(mc.want("tandem")) == 2
    res = mc.want("capacity")
    assert res["n_hits"].tolist() == [mc.LDS_CAPACITY, mc.LDS_CAPACITY + 1] and mc.n_wide(res) == 1


def test_fork_buckets():
    one, eight, default = mc.want("buckets_one"), mc.want("buckets_eight"), mc.want("k15_w10")
    assert (mc.index_entries(one["index"])[:, 0] == 0).all() and len(set(mc.index_entries(eight["index"])[:, 0].tolist())) == 8
    assert default["index"]["bucket_bits"] == 10
    for f in mc.FIELDS:
        assert np.array_equal(one[f], default[f]) and np.array_equal(eight[f], default[f])


def test_fork_unmapped():
    p = mc.get("unmapped")[0]
    res = mc.want("unmapped")
    assert res["n_hits"][0] == 0 and res["votes"].tolist() == [0, p["min_votes"] - 1, p["min_votes"]] and res["contig"].tolist() == [-1, -1, 0]


@pytest.mark.parametrize("wrong,name", [("rightmost", "homopolymer"), ("palindromes", "palindromes"), ("one_bin", "bins"), ("qa_is_q", "k15_w10"), ("tie_larger_contig", "identical_contigs"),
                                        ("second_adjacent", "bins"), ("occ_ge", "occ"), ("no_clip", "ends_extend1")])
def test_a_wrong_rule_gives_another_result(wrong, name):
    p, contigs, reads = mc.get(name)
    assert wrong in mc.WRONG and not mc.same(mc.want(name), mc.map_numpy(p, contigs, reads, wrong=wrong))


# ---- truth ----
def test_error_free_reads_map_to_exactly_their_origin():
    """inside a shared stretch the window minimizers of read and contig coincide: every hit lies on the true diagonal, and `extend` gives [s, s + Lr)"""
    p, c, reads, starts, strands = mc.exact_reads()
    res = mc.want("exact")
    assert min(len(r) for r in reads) == p["k"] + p["w"] - 1 and 0 in strands and 1 in strands
    for i, (r, s, st) in enumerate(zip(reads, starts, strands)):
        assert (res["contig"][i], res["strand"][i], res["qstart"][i], res["qend"][i], res["tstart"][i], res["tend"][i]) == (0, st, 0, len(r), s, s + len(r)), i


def noisy_case():
    """one contig of the dip10k kind: two haplotypes, ONT error, both strands, reads of 1 .. 3 kb"""
    from hairsplitter_amd import synth
    return synth.make_contig(41, 0, 10_000, 2, 0.01, 60, "ont", read_len_override=(1000, 3000))


def noisy_check(c, res):
    """every mapped read has its true span inside [tstart - 100, tend + 100) on the true contig and strand; at most 2 % unmapped"""
    from hairsplitter_amd import synth
    n_unmapped = 0
    for a in c.alns:
        i = a.read
        if res["contig"][i] < 0:
            n_unmapped += 1
            continue
        ops, lens = a.cigar & 0xF, a.cigar >> 4
        span = int(lens[(ops == synth.OP_M) | (ops == synth.OP_D) | (ops == synth.OP_EQ) | (ops == synth.OP_X)].sum())
        assert res["contig"][i] == 0 and bool(res["strand"][i]) == a.strand, i
        assert res["tstart"][i] - 100 <= a.pos and a.pos + span <= res["tend"][i] + 100, (i, a.pos, span, res["tstart"][i], res["tend"][i])
    assert n_unmapped <= 0.02 * len(c.alns), n_unmapped
    return n_unmapped


def test_noisy_reads_map_to_their_true_window():
    c = noisy_case()
    assert 200 <= len(c.reads) <= 600 and max(len(r) for r in c.reads) <= 3300
    noisy_check(c, mc.map_numpy(mc.params(), [c.seq], c.reads))
