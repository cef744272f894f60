"""Polishing passes on the device (hs_polish_refine_arrays, hs_polish_haplotypes_refined, hs_kernels_refine.hip). The yardstick is a
composition of entries that are held to their own oracles elsewhere: polish_refine_plan_host for pass p - 1, api.edlib_align(mode="NW", task="path") on
the coded pairs, run-length words in numpy, the host half with the consensus as backbone (tests/refine_cases.compose). (1) polish_refine with 1, 2 and 3
passes equals it on every case -- text, every per-bundle field, the per-pass sums, n_pairs, n_unaligned and sum_dist -- and the cases' claims hold;
(2) one pass is the planned route; (3) polish_haplotypes(passes=2) equals polish_refine on the inputs of the same job, and passes=1 is the one-pass
call in every field, its waits and its launches; (4) several sub-rounds equal one; (5) refusals; (6) the default step costs what it cost.

(7) the limit cases of tests/haplotype_cases.py -- op lengths of 2^16 and more, a CIGAR of exactly 2^31 - 1 bases, one of 2^31 refused -- through
one and two passes; (8) pass 2 and 3 over CIGARs the device wrote for noisy pieces, of more than 64 and more than 128 words, against the
composition; (9) A1 in several chunks equals one, several resident rounds with passes equal one; (10) one refusal and a call without pieces through
the four doors of the arrays (polish_consensus device and planned, polish_refine with one and two passes).

Limits not reached by a test: a piece above 2^20 bases (no path: the n_unaligned branch of k_refine_pieces) -- A1 sweeps the whole pair for its
distance before it declines the path, and nobody has measured that sweep; more than 2^31 - 256 pairs or 2^31 - 1 move bytes in an A1 chunk; more than
2^31 - 256 pieces, bundles or records; 2^30 columns. (A CIGAR beyond 2^31 - 1 bases IS reached, in milliseconds: a word holds 2^28 - 1, a D op needs no bases.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import consensus_cases as cc
import haplotype_cases as hc
import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CONS_KEYS = ("cons_off", "cons") + cc.FIELDS
_YARD = {}


def device_align(pairs):
    from hairsplitter_amd import api
    return [(r["ops"], r["distance"]) for r in api.edlib_align(pairs, mode="NW", task="path")]


def yardstick(group, params=None, key=None, passes=3):
    """three passes (or `passes`) of the composition on a case group, computed once and left unchanged"""
    from hairsplitter_amd import api
    key = key or group
    if key not in _YARD:
        bundles = dict(rc.CASES, **rc.NOISY, **hc.LIMIT_CASES)[group]()
        _YARD[key] = (bundles, cc.pack(bundles), rc.compose(cc.pack(bundles), passes, lambda job, prm: api.polish_refine_plan_host(job, prm), device_align, params))
    return _YARD[key]


def assert_pass_equals(dev, want, what):
    p = dev["passes"]["n_passes"]
    last = want[p - 1]["res"]
    for k in CONS_KEYS:
        assert np.array_equal(dev[k], last[k]), (what, p, k)
    for k in ("n_ins_records", "n_ins_slots"):
        assert dev["stats"][k] == last["stats"][k], (what, p, k)
    for q in range(p):
        for k in rc.SUMS:
            assert int(dev["passes"][k][q]) == int(want[q]["res"][k].sum()), (what, p, "pass", q + 1, k)
        for k in ("n_pairs", "n_unaligned", "sum_dist"):
            assert int(dev["passes"][k][q]) == want[q][k], (what, p, "pass", q + 1, k)


@pytest.mark.parametrize("group", sorted(rc.CASES))
def test_passes_equal_the_composition_on_every_case(built, group):
    from hairsplitter_amd import api
    bundles, job, want = yardstick(group)
    for p, x in enumerate(want):
        rc.check_pass_claims(bundles, p + 1, x["res"])
    for passes in (1, 2, 3):
        dev = api.polish_refine(job, passes=passes)
        assert_pass_equals(dev, want, group)
        if passes > 1:
            st = dev["passes"]
            print(group, passes, {k: st[k].tolist() for k in ("n_pairs", "sum_dist", "move_bytes", "cigar_words", "n_waits")})
            assert st["n_unaligned"].sum() == 0 and st["n_pairs"][0] == 0 and st["sum_dist"][0] == 0
            assert all(st["move_bytes"][1:] >= st["n_pairs"][1:]) and all(st["cigar_words"][1:] >= st["n_pairs"][1:] - st["n_unaligned"][1:])


def test_scattered_indels_are_found_by_the_second_pass_and_no_one_pass_call_has_that_text(built):
    from hairsplitter_amd import api
    bundles = rc.scattered_cases()
    job = cc.pack(bundles)
    one, two, three = (api.polish_refine(job, passes=p) for p in (1, 2, 3))
    for p, res in ((1, one), (2, two), (3, three)):
        rc.check_pass_claims(bundles, p, res)
    text = lambda r, i: api.consensus_text(r, i)
    assert text(one, 0) == bundles[0].backbone and text(two, 0) == rc.PRE + "GGGG" + rc.POST == text(three, 0)
    assert text(one, 2) == bundles[2].backbone and text(two, 2) == rc.PRE + "GGGG" + rc.POST == text(three, 2)
    assert two["passes"]["n_ins_bases"].tolist() == [2, 2] and two["passes"]["n_del"].tolist() == [0, 2]      # (bundle 1 inserts in pass 1, bundle 0 in pass 2)
    assert three["passes"]["n_ins_bases"].tolist() == [2, 2, 0] and three["passes"]["n_del"].tolist() == [0, 2, 0] and three["passes"]["sum_dist"].tolist() == [0, 12, 0]
    assert api.consensus_text(two, 0, trimmed=True) == (rc.PRE + "GGGG" + rc.POST)[2:12]


def test_other_parameters(built):
    from hairsplitter_amd import api
    for min_cov, max_ins in ((1, 2), (4, 64)):
        prm = api.consensus_params(min_cov=min_cov, max_ins=max_ins)
        _, job, want = yardstick("window_edges", prm, key=("window_edges", min_cov, max_ins))
        assert_pass_equals(api.polish_refine(job, prm, passes=3), want, (min_cov, max_ins))


def test_one_pass_is_the_planned_route(built):
    from hairsplitter_amd import api
    for group in sorted(rc.CASES):
        job = cc.pack(rc.CASES[group]())
        w0 = api.host_waits()
        planned = api.polish_consensus(job, form="planned")
        w1 = api.host_waits()
        one = api.polish_refine(job, passes=1)
        w2 = api.host_waits()
        for k in CONS_KEYS:
            assert np.array_equal(one[k], planned[k]), (group, k)
        assert one["passes"]["n_passes"] == 1 and int(one["passes"]["n_waits"][0]) == w2 - w1 == w1 - w0
        for k in rc.SUMS:
            assert int(one["passes"][k][0]) == int(planned[k].sum())


# ---- the job tests/test_gpu_haplotypes.py builds its batch from, restated -------------------------------------------------------------------
def diploid_contig():
    from hairsplitter_amd import synth
    return synth.make_contig(11, 0, 10_000, 2, 0.01, 60, "ont")


def labelled(contigs):
    """every read labelled by its haplotype in five windows of 2 000 columns"""
    c = contigs[0]
    n, k = len(c.alns), len(contigs)
    labels = np.array([c.haplotype_of_read[a.read] for a in c.alns], np.int32)
    return {"win_off": np.arange(k + 1, dtype=np.int64) * 5, "win_start": np.tile(np.arange(5, dtype=np.int32) * 2000, k),
            "win_end": np.tile(np.arange(5, dtype=np.int32) * 2000 + 1999, k), "label_off": np.arange(5 * k + 1, dtype=np.int64) * n, "labels": np.tile(labels, 5 * k)}


def test_haplotypes_with_passes_equal_the_arrays_route_and_one_pass_is_the_old_call(built):
    from hairsplitter_amd import api
    c = diploid_contig()
    batch = api.CvBatch(api.FlatBatch([c]))
    try:
        sr = labelled([c])
        inputs = api.polish_inputs(batch, sr, contig_has_snps=[1])
        arrays = api.polish_refine(inputs, passes=2)
        hap2 = api.polish_haplotypes(batch, sr, contig_has_snps=[1], passes=2)
        for k in CONS_KEYS:
            assert np.array_equal(hap2[k], arrays[k]), k
        for k in rc.SUMS + ("n_pairs", "n_unaligned", "sum_dist", "move_bytes", "cigar_words"):
            assert hap2["passes"][k].tolist() == arrays["passes"][k].tolist(), k
        print("passes", {k: hap2["passes"][k].tolist() for k in hap2["passes"] if k != "n_passes"})
        assert hap2["passes"]["n_pairs"][1] > 0 and not any(k in hap2 for k in ("backbone", "bases", "cigar"))
        # one pass through the new argument and through the new entry: the old call in every field, its waits and its launches
        api.kernel_stats_every(1)
        cost = []
        res = []
        for call in (lambda: api.polish_haplotypes(batch, sr, contig_has_snps=[1]), lambda: api.polish_haplotypes(batch, sr, contig_has_snps=[1], passes=1),
                     lambda: _refined_entry_one_pass(api, batch, sr)):
            api.kernel_stats_reset()
            w0 = api.host_waits()
            res.append(call())
            cost.append((api.host_waits() - w0, {k: v["launches"] for k, v in api.kernel_stats().items()}))
        assert cost[0] == cost[1] == cost[2], cost
        for other in res[1:]:
            for k in res[0]:
                if k not in ("stats", "passes"):
                    assert np.array_equal(res[0][k], other[k]), k
            for k in ("n_rounds", "n_sub_rounds", "bytes_down", "bytes_up", "n_ins_records", "n_ins_slots"):
                assert res[0]["stats"][k] == other["stats"][k], k
        assert res[2]["passes"]["n_passes"] == 1 and int(res[2]["passes"]["n_waits"][0]) == cost[2][0]
    finally:
        batch.close()


def _refined_entry_one_pass(api, batch, sr):
    """hs_polish_haplotypes_refined with n_passes = 1 (api.polish_haplotypes(passes=1) calls the old entry itself)"""
    import ctypes as C
    lib = api.load()
    arr = {k: np.ascontiguousarray(sr[k], np.int64 if k.endswith("_off") else np.int32) for k in ("win_off", "win_start", "win_end", "label_off", "labels")}
    has = np.ones(1, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out_p = C.POINTER(api.RefinedResult)()
    lib.hs_polish_haplotypes_refined.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.POINTER(api.RefinedResult))]
    lib.hs_refined_result_destroy.argtypes = [C.c_void_p]
    lib.hs_refined_result_destroy.restype = None
    api._check(lib.hs_polish_haplotypes_refined(batch.handle, 0, batch.flat.n_contigs, ptr(arr["win_off"]), ptr(arr["win_start"]), ptr(arr["win_end"]), ptr(arr["label_off"]),
                                                ptr(arr["labels"]), ptr(has), 0, None, 1, C.byref(out_p)))
    try:
        return api._haplotypes_result_dict(out_p.contents.last.contents, out_p.contents)
    finally:
        lib.hs_refined_result_destroy(out_p)


def test_several_sub_rounds_equal_one(built, monkeypatch):
    from hairsplitter_amd import api
    job = cc.pack(rc.rounds_cases())
    one = api.polish_refine(job, passes=3)
    assert one["stats"]["n_sub_rounds"] == 1
    monkeypatch.setenv("HS_CONSENSUS_CHUNK_MB", "1")
    many = api.polish_refine(job, passes=3)
    assert many["stats"]["n_sub_rounds"] >= 2
    for k in CONS_KEYS:
        assert np.array_equal(one[k], many[k]), k
    for k in rc.SUMS + ("n_pairs", "n_unaligned", "sum_dist", "move_bytes", "cigar_words"):
        assert one["passes"][k].tolist() == many["passes"][k].tolist(), k
    assert many["passes"]["n_waits"][1] > one["passes"]["n_waits"][1]
    rc.check_pass_claims(rc.rounds_cases(), 3, many)


# ---- 7. the limits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(hc.LIMIT_CASES))
def test_limit_cases_through_one_and_two_passes_equal_the_composition(built, group):
    """pass 2 there realigns short pieces against short texts (but for the long M bundles: 135 546 bases against 65 578)"""
    from hairsplitter_amd import api
    bundles, job, want = yardstick(group, passes=2)
    cc.check_claims(bundles, cc.result_as_rule(want[0]["res"]))
    for passes in (1, 2):
        dev = api.polish_refine(job, passes=passes)
        assert_pass_equals(dev, want, (group, [b.aim for b in bundles]))
    assert int(dev["passes"]["n_unaligned"].sum()) == 0 and int(dev["passes"]["n_pairs"][1]) > 0


@pytest.mark.parametrize("case", range(len(hc.refused_cases())))
def test_a_cigar_over_the_limit_is_refused_by_one_and_by_two_passes(built, case):
    from hairsplitter_amd import api
    name, bundles, named = hc.refused_cases()[case]
    job = cc.pack(bundles)
    for passes in (1, 2, 1, 2):
        with pytest.raises(api.HsError, match=r"bundle %d: a CIGAR of more than 2\^31 - 1 bases" % named):
            api.polish_refine(job, passes=passes)


# ---- 8. noisy pieces -------------------------------------------------------------------------------------------------------------------------
def test_noisy_pieces_equal_the_composition_over_cigars_the_device_wrote(built):
    """The conditions are read off the yardstick's own pass-2 job, not off the route under test: CIGARs of the k_m2c_* kernels with more than two
    64-op chunks and with more than one feed k_refine_pieces, k_cons_plan and k_cons_rows."""
    from hairsplitter_amd import api
    bundles, job, want = yardstick("noisy")
    n_words = np.diff(want[1]["job"]["cig_off"])
    print("noisy: words a piece in pass 2", sorted(n_words.tolist()), "sum_dist", [w["sum_dist"] for w in want])
    assert n_words.max() >= 129 and ((n_words >= 65) & (n_words <= 128)).any() and want[1]["sum_dist"] > 0
    assert len(bundles) == 2 and all(len(b.pieces) == 12 for b in bundles)
    for passes in (1, 2, 3):
        assert_pass_equals(api.polish_refine(job, passes=passes), want, "noisy")


# ---- 9. seams --------------------------------------------------------------------------------------------------------------------------------
PASS_KEYS = rc.SUMS + ("n_pairs", "n_unaligned", "sum_dist", "move_bytes", "cigar_words")

A1_CHILD = """
import sys
import numpy as np
sys.path.insert(0, "tests")
import consensus_cases as cc
import refine_cases as rc
import test_gpu_refine as tr
from hairsplitter_amd import api
res = api.polish_refine(cc.pack(rc.a1_chunks_cases()[0]), passes=2)
out = {k: np.asarray(res[k]) for k in tr.CONS_KEYS}
out.update({"pass_" + k: res["passes"][k] for k in tr.PASS_KEYS + ("n_waits",)})
np.savez(sys.argv[1], **out)
"""


def test_a1_in_several_chunks_equals_one(built, tmp_path):
    """HS_REALIGN_CHUNK_MB is read once a process: a child runs the job under 16 (the floor; queries plus windows are 19.2 MB, two chunks), this process
    under the default (one). A wait per chunk. Measured on an MI355X: the call 0.04 s in this process (A1 over the 2 400 pairs: 13 ms), the child 2.1 s with its start, the
    test 2.2 s."""
    import time
    from hairsplitter_amd import api
    bundles, haps = rc.a1_chunks_cases()
    job = cc.pack(bundles)
    assert int(job["base_off"][-1]) + sum(len(b.backbone) * len(b.pieces) for b in bundles) > 16 << 20
    t0 = time.perf_counter()
    one = api.polish_refine(job, passes=2)
    print("a1 chunks job: polish_refine(passes=2) in this process %.2f s" % (time.perf_counter() - t0), {k: one["passes"][k].tolist() for k in ("n_pairs", "n_waits", "align_ms")})
    dst = str(tmp_path / "child.npz")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", A1_CHILD, dst], cwd=ROOT, env=dict(os.environ, HS_REALIGN_CHUNK_MB="16"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print("a1 chunks job: the child %.2f s" % (time.perf_counter() - t0))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    child = np.load(dst)
    for k in CONS_KEYS:
        assert np.array_equal(one[k], child[k]), k
    for k in PASS_KEYS:
        assert one["passes"][k].tolist() == child["pass_" + k].tolist(), k
    assert int(child["pass_n_waits"][1]) >= int(one["passes"]["n_waits"][1]) + 1 and int(child["pass_n_waits"][0]) == int(one["passes"]["n_waits"][0])
    assert one["stats"]["n_sub_rounds"] == 1 and int(one["passes"]["n_pairs"][1]) == sum(len(b.pieces) for b in bundles)
    assert [api.consensus_text(one, i) for i in range(len(bundles))] == haps


def three_contigs_two_passes(api):
    c = diploid_contig()
    batch = api.CvBatch(api.FlatBatch([c, c, c]))
    try:
        return api.polish_haplotypes(batch, labelled([c, c, c]), contig_has_snps=[1, 1, 1], passes=2)
    finally:
        batch.close()


ROUNDS_CHILD = """
import sys
import numpy as np
sys.path.insert(0, "tests")
import test_gpu_haplotypes as th
import test_gpu_refine as tr
from hairsplitter_amd import api
res = tr.three_contigs_two_passes(api)
out = {k: np.asarray(res[k]) for k in th.CONS_KEYS + th.META_KEYS}
out.update({k: np.int64(res["stats"][k]) for k in th.COUNTS + ("n_rounds", "n_sub_rounds")})
out.update({"pass_" + k: res["passes"][k] for k in tr.PASS_KEYS})
np.savez(sys.argv[1], **out)
"""


def test_several_resident_rounds_and_several_sub_rounds_with_passes_equal_one(built, tmp_path):
    """RefineStats accumulates over the resident rounds and refine_first_pass subtracts the later passes' waits from the call's: every per-pass sum
    but n_waits (which legitimately differs) is that of the one-round call"""
    from hairsplitter_amd import api
    from test_gpu_haplotypes import COUNTS, META_KEYS
    one = three_contigs_two_passes(api)
    assert one["stats"]["n_rounds"] == 1 and one["stats"]["n_sub_rounds"] == 1 and one["n_bundles"] >= 6 and int(one["passes"]["n_pairs"][1]) > 0
    for env, check in (({"HS_POLISH_CHUNK_MB": "1"}, lambda r, s: r >= 2 and s >= r), ({"HS_CONSENSUS_CHUNK_MB": "1"}, lambda r, s: r == 1 and s > r)):
        dst = str(tmp_path / ("child_%s.npz" % list(env)[0]))
        r = subprocess.run([sys.executable, "-c", ROUNDS_CHILD, dst], cwd=ROOT, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        child = np.load(dst)
        assert check(int(child["n_rounds"]), int(child["n_sub_rounds"])), (env, int(child["n_rounds"]), int(child["n_sub_rounds"]))
        for k in CONS_KEYS + META_KEYS:
            assert np.array_equal(one[k], child[k]), (env, k)
        for k in COUNTS:
            assert one["stats"][k] == int(child[k]), (env, k)
        for k in PASS_KEYS:
            assert one["passes"][k].tolist() == child["pass_" + k].tolist(), (env, k)


def test_tool_writes_the_refined_fasta_under_hs_polish_passes(built, tmp_path):
    """HS_HAPLOTYPES=1 HS_POLISH_PASSES=2: the FASTA of polish_haplotypes_from_files(passes=2); unset or 1: today's file; outside 1..8: non-zero, by name"""
    import os
    import subprocess
    import polish_goldens as pg
    from hairsplitter_amd import api
    tool = built["polish_inputs"]
    env = {k: v for k, v in os.environ.items() if k not in ("HS_HAPLOTYPES", "HS_CONSENSUS", "HS_POLISH_PASSES")}
    gfa, reads, sam, gro = pg.prepare("multi", str(tmp_path))
    out = {k: str(tmp_path / (k + ".fa")) for k in ("unset", "one", "two", "api1", "api2", "bad")}
    for k, extra in (("unset", {}), ("one", {"HS_POLISH_PASSES": "1"}), ("two", {"HS_POLISH_PASSES": "2"})):
        r = subprocess.run([tool, gfa, reads, sam, gro, "1", out[k]], env=dict(env, HS_HAPLOTYPES="1", **extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
    api.polish_haplotypes_from_files(gfa, reads, sam, gro, out["api1"], polish_everything=True)
    api.polish_haplotypes_from_files(gfa, reads, sam, gro, out["api2"], polish_everything=True, passes=2)
    text = {k: open(out[k]).read() for k in ("unset", "one", "two", "api1", "api2")}
    assert text["unset"] == text["one"] == text["api1"] and text["two"] == text["api2"]
    assert text["two"].count(">") == text["one"].count(">") > 0
    for bad in ("0", "9", "two"):
        r = subprocess.run([tool, gfa, reads, sam, gro, "1", out["bad"]], env=dict(env, HS_HAPLOTYPES="1", HS_POLISH_PASSES=bad), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode != 0 and b"allowed 1..8" in r.stdout and not os.path.exists(out["bad"]), (bad, r.stdout.decode()[-500:])


def test_refusals(built):
    from hairsplitter_amd import api
    job = cc.pack(rc.scattered_cases())
    for n in (0, 9, -1):
        with pytest.raises(api.HsError, match=r"n_passes is %d, allowed 1\.\.8" % n):
            api.polish_refine(job, passes=n)
    c = diploid_contig()
    batch = api.CvBatch(api.FlatBatch([c]))
    try:
        for n in (0, 9):
            with pytest.raises(api.HsError, match=r"n_passes is %d, allowed 1\.\.8" % n):
                api.polish_haplotypes(batch, labelled([c]), contig_has_snps=[1], passes=n)
    finally:
        batch.close()
    with pytest.raises(api.HsError, match="out of range"):
        api.polish_refine(job, api.consensus_params(max_ins=65), passes=2)


# ---- 10. the four doors of the arrays: one checked input, one plan step, one cutter behind them ------------------------------------------------
DOORS = (("hs_polish_consensus", lambda api, job: api.polish_consensus(job, form="device")),
         ("hs_polish_consensus_planned_tap", lambda api, job: api.polish_consensus(job, form="planned")),
         ("hs_polish_refine_arrays", lambda api, job: api.polish_refine(job, passes=1)),
         ("hs_polish_refine_arrays", lambda api, job: api.polish_refine(job, passes=2)))


def test_one_refusal_through_every_door(built):
    """An input hs::consensus_check rejects and a CIGAR of 2^31 bases (tests/haplotype_cases.py refused_cases, the long piece in bundle 2 of 3): behind the
    entry's own name the same text and status through all four doors -- the texts the calls gave before they shared their check and their plan step.
    The long CIGAR is refused by the host's plan without a wait and by the device's at its first wait: with two passes too, pass 1's plan, before any A1 launch."""
    import re
    from hairsplitter_amd import api
    good = cc.pack(cc.trim_cases())
    bad = dict(good, bundle_overhang_right=-np.ones_like(good["bundle_overhang_right"]))
    _, bundles, named = hc.refused_cases()[2]
    assert named == 2
    for job, status, text, waits in ((bad, -2, "bundle 0: a negative overhang", (0, 0, 0, 0)),
                                     (cc.pack(bundles), -2, "bundle 2: a CIGAR of more than 2^31 - 1 bases", (0, 1, 1, 1))):
        for (entry, call), n_waits in zip(DOORS, waits):
            w0 = api.host_waits()
            with pytest.raises(api.HsError) as e:
                call(api, job)
            m = re.fullmatch(r"hairsplitter_hip error (-?\d+): %s: (.*)" % entry, str(e.value))
            assert m and (int(m.group(1)), m.group(2)) == (status, text), (entry, str(e.value))
            assert api.host_waits() - w0 == n_waits, (entry, text)


def test_no_pieces_through_every_door(built):
    """No bundle at all, then two bundles with backbones and no piece, base_off and cig_off given as the one-element arrays such a call may pass: every
    door returns the backbones themselves, every column low where min_cov >= 1 asks for a piece, as the host half does; two passes realign no pair."""
    from hairsplitter_amd import api
    bundles = [cc.Bundle("300 columns, no piece", cc.seq(300, 5), [], ovl=3, ovr=4), cc.Bundle("7 columns, no piece", cc.seq(7, 6), [])]
    for some in ([], bundles):
        job = dict(cc.pack(some), base_off=np.zeros(1, np.int64), cig_off=np.zeros(1, np.int64))
        host = api.polish_consensus(job, form="host")
        assert [api.consensus_text(host, i) for i in range(len(some))] == [b.backbone for b in some]
        assert host["n_low"].tolist() == [len(b.backbone) for b in some] and not any(host[k].any() for k in ("n_sub", "n_del", "n_ins_bases", "n_skipped"))
        results = [call(api, job) for _, call in DOORS] + [api.polish_refine_plan_host(job)]
        for res in results:
            for k in CONS_KEYS:
                assert np.array_equal(res[k], host[k]), (len(some), k)
        assert results[3]["passes"]["n_pairs"].tolist() == [0, 0] and results[3]["passes"]["n_low"].tolist() == [int(host["n_low"].sum())] * 2
        assert len(results[4]["win_start"]) == 0


def test_default_step_costs_what_it_cost_before_a_refined_call(built):
    from hairsplitter_amd import api
    from test_gpu_alleles import _job
    from test_gpu_recruit import _step_cost
    pg = api.PipelineGroups(_job(), 2)
    try:
        before = _step_cost(pg, api)
        n = pg.flat.n_contigs
        sr = {"win_off": np.zeros(n + 1, np.int64), "win_start": np.zeros(0, np.int32), "win_end": np.zeros(0, np.int32), "label_off": np.zeros(1, np.int64),
              "labels": np.zeros(0, np.int32)}
        hap = api.polish_haplotypes(pg, sr, polish_everything=True, passes=2)
        assert 1 <= hap["n_bundles"] <= n and hap["passes"]["n_pairs"][1] > 0
        assert _step_cost(pg, api) == before
    finally:
        pg.close()
