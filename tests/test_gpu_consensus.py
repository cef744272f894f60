"""The bundle consensus on the device (hs_kernels_consensus.hip, hs_capi_consensus.inc): the device equals the host half of the rule
(hs_polish_consensus_host) on every case of tests/consensus_cases.py and every field by integer equality, twice; the wait count; one job in two
rounds and in one; the over-budget bundle; the round cutter at its seams on the host-planned and the resident route; polish_inputs -> polish_consensus on a resident batch; bin/hs_polish_inputs with HS_CONSENSUS=1;
k_cons_rows on op lengths of 2^16 and more and on a CIGAR of exactly 2^31 - 1 bases (tests/haplotype_cases.py LIMIT_CASES), where its plain int
scans run just below the bound the plan guards."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import consensus_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("cons_off", "cons") + cc.FIELDS
COUNTS = ("n_ins_records", "n_ins_slots")


def _same(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in COUNTS:
        assert a["stats"][k] == b["stats"][k], (what, k)


@pytest.mark.parametrize("group", sorted(cc.CASES))
def test_device_equals_the_host_half(built, group):
    from hairsplitter_amd import api
    bundles = cc.CASES[group]()
    job = cc.pack(bundles)
    host = api.polish_consensus(job, form="host")
    cc.check_claims(bundles, cc.result_as_rule(host))
    for run in (0, 1):      # (twice: nothing may hinge on the order in which the records' additions arrive)
        w0 = api.host_waits()
        dev = api.polish_consensus(job)
        assert api.host_waits() - w0 <= 3 * dev["stats"]["n_rounds"] and dev["stats"]["n_rounds"] == 1
        _same(dev, host, (group, run))


def test_rows_of_the_limit_cases_equal_the_run_length_rule(built):
    """every limit case in ONE call, behind a plain bundle: rows, records and columns of the cases at offsets other than 0"""
    import haplotype_cases as hc
    from hairsplitter_amd import api
    bundles = cc.trim_cases()[:1] + [b for g in sorted(hc.LIMIT_CASES) for b in hc.LIMIT_CASES[g]()]
    job = cc.pack(bundles)
    want = cc.rule_rl(job)
    cc.check_claims(bundles, want)
    for run in (0, 1):
        dev = api.polish_consensus(job)
        cc.assert_same(cc.result_as_rule(dev), want, (run, [(b.name, getattr(b, "aim", "")) for b in bundles]))
        assert dev["stats"]["n_rounds"] == 1


def test_other_parameters(built):
    from hairsplitter_amd import api
    job = cc.pack(cc.slots_cases() + cc.edges_cases())
    for min_cov, max_ins in ((1, 2), (4, 64), (2, 1)):
        prm = api.consensus_params(min_cov=min_cov, max_ins=max_ins)
        _same(api.polish_consensus(job, prm), api.polish_consensus(job, prm, form="host"), (min_cov, max_ins))


def test_refused_input(built):
    from hairsplitter_amd import api
    job = cc.pack(cc.trim_cases())
    for kw in ({"min_cov": 0}, {"max_ins": 0}, {"max_ins": 65}):
        for form in ("device", "host"):
            with pytest.raises(api.HsError, match="out of range"):
                api.polish_consensus(job, api.consensus_params(**kw), form=form)
    bad = dict(job, piece_sam_pos=np.zeros_like(job["piece_sam_pos"]))
    with pytest.raises(api.HsError, match="start position"):
        api.polish_consensus(bad)


def two_round_job():
    """two bundles of 7 000 columns under 100 pieces each: 700 000 row bytes a bundle, so that a budget of 1 MB holds one"""
    out = []
    for k in (0, 1):
        bb = cc.seq(7000, 70 + k)
        text = bb[:3500] + "GT" + bb[3500:5000] + bb[5002:]
        out.append(cc.Bundle("half %d" % k, bb, [(1, "3500M2I1500M2D1998M", text)] * 60 + [(1, "7000M", bb)] * 40, ovl=150, ovr=150))
    return out


CHILD = """
import sys
import numpy as np
sys.path.insert(0, "tests")
import consensus_cases as cc
import test_gpu_consensus as tg
from hairsplitter_amd import api
job = cc.pack(tg.two_round_job())
res = api.polish_consensus(job)
out = {k: np.asarray(res[k]) for k in tg.KEYS}
out.update({k: np.int64(res["stats"][k]) for k in tg.COUNTS + ("n_rounds",)})
big = cc.pack([cc.Bundle("big", cc.seq(7000, 1), [(1, "7000M", cc.seq(7000, 1))] * 160)])
try:
    api.polish_consensus(big)
    out["refused"] = np.array("")
except api.HsError as e:
    out["refused"] = np.array(str(e))
np.savez(sys.argv[1], **out)
"""


def test_two_rounds_equal_one_round_and_the_bundle_above_the_budget_is_refused(built, tmp_path):
    from hairsplitter_amd import api
    dst = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, dst], cwd=ROOT, env=dict(os.environ, HS_CONSENSUS_CHUNK_MB="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    child = np.load(dst)
    job = cc.pack(two_round_job())
    w0 = api.host_waits()
    one = api.polish_consensus(job)
    assert api.host_waits() - w0 <= 3
    assert int(child["n_rounds"]) == 2 and one["stats"]["n_rounds"] == 1
    for k in KEYS:
        assert np.array_equal(one[k], child[k]), k
    for k in COUNTS:
        assert one["stats"][k] == int(child[k]), k
    assert one["n_ins_bases"].tolist() == [2, 2] and one["n_del"].tolist() == [2, 2]
    _same(one, api.polish_consensus(job, form="host"))
    msg = str(child["refused"])
    assert "bundle 0" in msg and "HS_CONSENSUS_CHUNK_MB" in msg, msg


BUDGET = 1 << 20      # HS_CONSENSUS_CHUNK_MB=1


def rounds_by_rule(row_bytes, budget=BUDGET):
    """whole bundles in order; a bundle opens a round where the round before would exceed the budget with it"""
    n, used = 0, budget + 1
    for rb in row_bytes:
        n, used = (n + 1, rb) if used + rb > budget else (n, used + rb)
    return n


def seam_bundle(n_pieces, L, seed):
    """n_pieces pieces of L columns, all M: n_pieces * L row bytes"""
    bb = cc.seq(L, seed)
    return cc.Bundle("%d x %d" % (n_pieces, L), bb, [(1, "%dM" % L, bb)] * n_pieces)


SEAM_BUNDLES = {"budget - 1": (1023, 1025), "budget": (1024, 1024), "one": (1, 1), "budget + 1": (17, 61681)}
SEAM_ORDERS = (("budget - 1", "budget", "one"), ("one", "budget - 1", "budget"), ("budget", "one", "budget - 1"))

SEAM_CHILD = """
import json
import sys
sys.path.insert(0, "tests")
import consensus_cases as cc
import test_gpu_consensus as tg
from hairsplitter_amd import api
out = {"rounds": [], "refused": []}
for order in tg.SEAM_ORDERS:
    job = cc.pack([tg.seam_bundle(*tg.SEAM_BUNDLES[k], seed=i) for i, k in enumerate(order)])
    dev, planned = api.polish_consensus(job, form="device"), api.polish_consensus(job, form="planned")
    tg._same(dev, planned, order)
    assert [len(api.consensus_text(dev, i)) for i in range(3)] == [tg.SEAM_BUNDLES[k][1] for k in order] and int(dev["n_sub"].sum()) == 0
    out["rounds"].append([dev["stats"]["n_rounds"], planned["stats"]["n_rounds"]])
big = cc.pack([tg.seam_bundle(*tg.SEAM_BUNDLES["one"], seed=1), tg.seam_bundle(*tg.SEAM_BUNDLES["budget + 1"], seed=2)])
for form in ("device", "planned"):
    try:
        api.polish_consensus(big, form=form)
        out["refused"].append("")
    except api.HsError as e:
        out["refused"].append(str(e))
json.dump(out, open(sys.argv[1], "w"))
"""


def test_the_round_cutter_at_its_seams_on_both_routes(built, tmp_path):
    """Row bytes of budget - 1, budget and 1 under HS_CONSENSUS_CHUNK_MB=1, in three orders: the host-planned route and the resident route cut the same
    rounds, those of the rule restated above (3, 2 and 2: the single byte joins a neighbour only beside budget - 1); one byte above the budget is
    refused by both, by name. A child, as the variable's other tests."""
    import json
    sizes = {k: n * L for k, (n, L) in SEAM_BUNDLES.items()}
    assert [sizes[k] for k in ("budget - 1", "budget", "one", "budget + 1")] == [BUDGET - 1, BUDGET, 1, BUDGET + 1]
    want = [rounds_by_rule([sizes[k] for k in order]) for order in SEAM_ORDERS]
    assert want == [3, 2, 2]
    dst = str(tmp_path / "child.json")
    r = subprocess.run([sys.executable, "-c", SEAM_CHILD, dst], cwd=ROOT, env=dict(os.environ, HS_CONSENSUS_CHUNK_MB="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    child = json.load(open(dst))
    assert child["rounds"] == [[n, n] for n in want], child["rounds"]
    for entry, msg in zip(("hs_polish_consensus", "hs_polish_consensus_planned_tap"), child["refused"]):
        assert msg.endswith("%s: bundle 1 alone takes %d row bytes, more than HS_CONSENSUS_CHUNK_MB allows" % (entry, BUDGET + 1)), msg


def test_polish_inputs_to_consensus_on_a_resident_batch(built):
    """the noisy diploid contig of tests/test_cpu_consensus.py as a resident batch: its reads labelled by their haplotype in five windows"""
    from hairsplitter_amd import api, synth
    c = synth.make_contig(11, 0, 10_000, 2, 0.01, 60, "ont")
    batch = api.CvBatch(api.FlatBatch([c]))
    n = len(c.alns)
    labels = np.array([c.haplotype_of_read[a.read] for a in c.alns], np.int32)
    sr = {"win_off": np.array([0, 5], np.int64), "win_start": np.arange(5, dtype=np.int32) * 2000, "win_end": np.arange(5, dtype=np.int32) * 2000 + 1999,
          "label_off": np.arange(6, dtype=np.int64) * n, "labels": np.tile(labels, 5)}
    res = api.polish_inputs(batch, sr, contig_has_snps=[1])
    assert res["n_bundles"] >= 2 and res["n_pieces"] + len(res["dropped"]) == n      # (every read has a label: it is a piece of its group's bundle, or dropped)
    dev, host = api.polish_consensus(res), api.polish_consensus(res, form="host")
    _same(dev, host)
    assert dev["stats"]["n_ins_records"] > 0 and int(dev["n_sub"].sum()) > 0
    batch.close()


def _parse_tool(path):
    """bin/hs_polish_inputs' text as bundles (the pieces it writes: the non-empty ones) and its consensus lines"""
    bundles, cons = [], []
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines):
        if lines[i].startswith("BUNDLE\t"):
            head = lines[i].split("\t")
            bundles.append(cc.Bundle(lines[i], lines[i + 2], [], int(head[7]), int(head[8])))
            i += 3
        elif lines[i].startswith(">read"):
            _, sam, cigar = lines[i].split(" ")
            bundles[-1].pieces.append((int(sam), cc.words(cigar), lines[i + 1], 0))
            i += 2
        elif lines[i].startswith(">consensus "):
            _, a, b = lines[i].split(" ")
            cons.append((int(a), int(b), lines[i + 1]))
            i += 2
        else:
            i += 1
    return bundles, cons


def test_tool_with_consensus_equals_the_api(built):
    import polish_goldens as pg
    from hairsplitter_amd import api
    with tempfile.TemporaryDirectory() as td:
        gfa, reads, sam, gro = pg.prepare("multi", td)
        out = os.path.join(td, "polish.txt")
        r = subprocess.run([built["polish_inputs"], gfa, reads, sam, gro, "1", out], env=dict(os.environ, HS_CONSENSUS="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        bundles, cons = _parse_tool(out)
        plain = os.path.join(td, "plain.txt")
        api.polish_inputs_from_files(gfa, reads, sam, gro, plain, polish_everything=True)
        assert ">consensus" not in open(plain).read()
    assert len(bundles) == len(cons) > 0 and sum(len(b.pieces) for b in bundles) > 0
    res = api.polish_consensus(cc.pack(bundles))
    got = [(int(res["trim_start"][i]), int(res["trim_end"][i]), api.consensus_text(res, i)) for i in range(len(bundles))]
    assert got == cons
