"""From labels to haplotype sequences on the device (hs_polish_haplotypes, k_cons_plan): (1) the plan of every piece as the device
finds it equals its numpy restatement, and the planned route equals the host half, on every case of tests/consensus_cases.py and
tests/haplotype_cases.py; (2) polish_haplotypes equals polish_consensus(polish_inputs(...)) and the host half on a noisy diploid contig, without
bringing the pieces down, within its host waits; (3) several resident rounds and several consensus sub-rounds equal one; (4) the FASTA of
bin/hs_polish_inputs under HS_HAPLOTYPES=1; (5) refusals; (6) the default pipeline step costs what it cost; (7) the limit cases of
tests/haplotype_cases.py: op lengths of 2^16 and more and a CIGAR whose M, I and D lengths sum to exactly 2^31 - 1 on the host half, the
host-planned route and the device-planned route, and one base more refused by all three, naming the same bundle (a CIGAR word holds 2^28 - 1 and
a D op needs no bases: the limit is reached in milliseconds).

Limits not reached by a test: more than 2^31 - 256 pieces or bundles in a resident round, more than 2^31 - 256 insertion records or 2^30 columns
in a sub-round."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import consensus_cases as cc
import haplotype_cases as hc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONS_KEYS = ("cons_off", "cons") + cc.FIELDS
COUNTS = ("n_ins_records", "n_ins_slots")
META_KEYS = ("n_bundles", "n_pieces", "bundle_contig", "bundle_interval", "bundle_start", "bundle_end", "bundle_group", "bundle_left_to_polish", "bundle_right_to_polish",
             "bundle_overhang_left", "bundle_overhang_right", "piece_rec", "piece_read_start", "piece_read_end", "piece_sam_pos", "piece_flags", "backbone_off", "piece_off",
             "base_off", "cig_off", "dropped")
GROUPS = dict(hc.all_groups())


def _same(a, b, what=""):
    for k in CONS_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in COUNTS:
        assert a["stats"][k] == b["stats"][k], (what, k)


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_device_plan_equals_its_restatement_and_the_planned_route_the_host_half(built, group):
    from hairsplitter_amd import api
    bundles = GROUPS[group]
    job = cc.pack(bundles)
    host = api.polish_consensus(job, form="host")
    cc.check_claims(bundles, cc.result_as_rule(host))
    want, _ = hc.piece_plan(job)
    for run in (0, 1):      # (twice: nothing may hinge on the order in which the pieces' additions arrive)
        w0 = api.host_waits()
        dev = api.polish_consensus(job, form="planned")
        waits = api.host_waits() - w0
        assert np.array_equal(dev["plan"], want), (group, run, np.flatnonzero((dev["plan"] != want).any(axis=1))[:8])
        _same(dev, host, (group, run))
        assert dev["stats"]["n_rounds"] == (1 if len(bundles) else 0) and waits == 1 + 2 * dev["stats"]["n_rounds"]      # (one wait for the sizes, two a round: measured on every group)


def test_planned_route_with_other_parameters(built):
    from hairsplitter_amd import api
    job = cc.pack(cc.slots_cases() + cc.edges_cases() + hc.chunk_edge_cases() + hc.room_cases())
    for min_cov, max_ins in ((1, 2), (4, 64), (2, 1)):
        prm = api.consensus_params(min_cov=min_cov, max_ins=max_ins)
        _same(api.polish_consensus(job, prm, form="planned"), api.polish_consensus(job, prm, form="host"), (min_cov, max_ins))


# ---- 2. the composition --------------------------------------------------------------------------------------------------------------------
def diploid_contig():
    """the noisy 10-kb diploid contig of test_gpu_consensus.test_polish_inputs_to_consensus_on_a_resident_batch and its labels in five windows"""
    from hairsplitter_amd import synth
    return synth.make_contig(11, 0, 10_000, 2, 0.01, 60, "ont")


def labelled(contigs):
    """sr of `contigs` (copies of one contig): every read labelled by its haplotype in five windows of 2 000 columns"""
    c = contigs[0]
    n, k = len(c.alns), len(contigs)
    labels = np.array([c.haplotype_of_read[a.read] for a in c.alns], np.int32)
    return {"win_off": np.arange(k + 1, dtype=np.int64) * 5, "win_start": np.tile(np.arange(5, dtype=np.int32) * 2000, k),
            "win_end": np.tile(np.arange(5, dtype=np.int32) * 2000 + 1999, k), "label_off": np.arange(5 * k + 1, dtype=np.int64) * n, "labels": np.tile(labels, 5 * k)}


def test_haplotypes_equal_the_two_calls_and_the_host_half_without_the_pieces_coming_down(built):
    """The wait bound is that of a batch whose record tables are on the host already: the first polishing call on a batch fetches them once (one more
    wait), and polish_inputs has been that call here."""
    from hairsplitter_amd import api
    c = diploid_contig()
    batch = api.CvBatch(api.FlatBatch([c]))
    try:
        sr = labelled([c])
        inputs = api.polish_inputs(batch, sr, contig_has_snps=[1])
        two = api.polish_consensus(inputs)
        host = api.polish_consensus(inputs, form="host")
        for run in (0, 1):
            w0 = api.host_waits()
            hap = api.polish_haplotypes(batch, sr, contig_has_snps=[1])
            waits = api.host_waits() - w0
            st = hap["stats"]
            _same(hap, two, run)
            _same(hap, host, run)
            for k in META_KEYS:
                assert np.array_equal(hap[k], inputs[k]), k
            assert not any(k in hap for k in ("backbone", "bases", "cigar"))
            assert st["n_rounds"] == 1 and st["n_sub_rounds"] == 1 and st["cut_ops_read"] == inputs["stats"]["cut_ops_read"] and st["n_tasks"] == inputs["stats"]["n_tasks"]
            print("waits", waits, "bytes_down", st["bytes_down"], "bytes_up", st["bytes_up"], "bases", int(inputs["base_off"][-1]), "plan_ms", st["plan_ms"])
            assert waits == 1 + st["n_rounds"] + 2 * st["n_sub_rounds"], waits      # (measured: 4)
            assert 0 < st["bytes_down"] < int(inputs["base_off"][-1])      # (the cut table and the text: tens of KB; the bases alone are 600 KB)
        assert hap["n_bundles"] >= 2 and st["n_ins_records"] > 0 and int(hap["n_sub"].sum()) > 0
        for i in range(hap["n_bundles"]):
            o = int(two["cons_off"][i])
            assert api.haplotype_text(hap, i) == two["cons"][o + int(two["trim_start"][i]):o + int(two["trim_end"][i])].tobytes().decode()
            assert len(api.haplotype_text(hap, i)) > 1000
    finally:
        batch.close()


# ---- 3. rounds -----------------------------------------------------------------------------------------------------------------------------
def three_contigs_result(api):
    c = diploid_contig()
    batch = api.CvBatch(api.FlatBatch([c, c, c]))
    try:
        return api.polish_haplotypes(batch, labelled([c, c, c]), contig_has_snps=[1, 1, 1])
    finally:
        batch.close()


CHILD = """
import sys
import numpy as np
sys.path.insert(0, "tests")
import test_gpu_haplotypes as th
from hairsplitter_amd import api
res = th.three_contigs_result(api)
out = {k: np.asarray(res[k]) for k in th.CONS_KEYS + th.META_KEYS}
out.update({k: np.int64(res["stats"][k]) for k in th.COUNTS + ("n_rounds", "n_sub_rounds")})
np.savez(sys.argv[1], **out)
"""


def test_several_rounds_and_several_sub_rounds_equal_one(built, tmp_path):
    from hairsplitter_amd import api
    one = three_contigs_result(api)
    assert one["stats"]["n_rounds"] == 1 and one["stats"]["n_sub_rounds"] == 1 and one["n_bundles"] >= 6
    for env, check in (({"HS_POLISH_CHUNK_MB": "1"}, lambda r, s: r >= 2 and s >= r), ({"HS_CONSENSUS_CHUNK_MB": "1"}, lambda r, s: r == 1 and s > r)):
        dst = str(tmp_path / ("child_%s.npz" % list(env)[0]))
        r = subprocess.run([sys.executable, "-c", CHILD, dst], cwd=ROOT, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        child = np.load(dst)
        assert check(int(child["n_rounds"]), int(child["n_sub_rounds"])), (env, int(child["n_rounds"]), int(child["n_sub_rounds"]))
        for k in CONS_KEYS + META_KEYS:
            assert np.array_equal(one[k], child[k]), (env, k)
        for k in COUNTS:
            assert one["stats"][k] == int(child[k]), (env, k)


# ---- 4. files ------------------------------------------------------------------------------------------------------------------------------
def _fasta(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    assert all(h.startswith(">") for h in lines[0:-1:2])
    return list(zip(lines[0:-1:2], lines[1:-1:2]))


@pytest.mark.parametrize("polish", (0, 1))
@pytest.mark.parametrize("case", ("multi", "clips", "edge_ops"))
def test_tool_writes_the_trimmed_consensus_of_every_bundle_as_fasta(built, case, polish):
    import polish_goldens as pg
    from hairsplitter_amd import api
    from test_gpu_consensus import _parse_tool
    tool = built["polish_inputs"]
    env = {k: v for k, v in os.environ.items() if k not in ("HS_HAPLOTYPES", "HS_CONSENSUS")}
    with tempfile.TemporaryDirectory() as td:
        gfa, reads, sam, gro = pg.prepare(case, td)
        out = {k: os.path.join(td, k + ".txt") for k in ("plain", "cons", "hap", "both", "api", "api_plain")}
        for k, extra in (("plain", {}), ("cons", {"HS_CONSENSUS": "1"}), ("hap", {"HS_HAPLOTYPES": "1"}), ("both", {"HS_HAPLOTYPES": "1", "HS_CONSENSUS": "1"})):
            r = subprocess.run([tool, gfa, reads, sam, gro, str(polish), out[k]], env=dict(env, **extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            assert r.returncode == 0, r.stdout.decode()[-2000:]
        api.polish_haplotypes_from_files(gfa, reads, sam, gro, out["api"], polish_everything=bool(polish))
        hap = _fasta(out["hap"])
        assert open(out["both"]).read() == open(out["hap"]).read()      # HS_HAPLOTYPES wins over HS_CONSENSUS
        assert open(out["api"]).read() == open(out["hap"]).read()
        bundles, cons = _parse_tool(out["cons"])
        want = []
        for b, (a, e, text) in zip(bundles, cons):
            head = b.name.split("\t")      # BUNDLE, contig, start, end, group, ...
            want.append((">%s_%s_%s_%s" % (head[1], head[2], head[3], head[4]), text[a:max(a, e)]))
        assert len(bundles) == len(cons) and hap == want
        # without either variable: the text of today -- the consensus text without its consensus lines
        plain = open(out["plain"]).read()
        assert ">consensus" not in plain and not plain.startswith(">")
        kept, lines, i = [], open(out["cons"]).read().split("\n"), 0
        while i < len(lines):
            if lines[i].startswith(">consensus "):
                i += 2
            else:
                kept.append(lines[i])
                i += 1
        assert "\n".join(kept) == plain
        if polish:
            assert len(hap) > 0 and any(len(t) > 0 for _, t in hap)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(built, monkeypatch):
    from hairsplitter_amd import api, synth
    c = synth.make_contig(11, 0, 20_000, 1, 0.0, 60, "ont")      # one bundle over the whole contig: 20 000 columns under some 60 pieces
    batch = api.CvBatch(api.FlatBatch([c]))
    sr = {"win_off": np.zeros(2, np.int64), "win_start": np.zeros(0, np.int32), "win_end": np.zeros(0, np.int32), "label_off": np.zeros(1, np.int64),
          "labels": np.zeros(0, np.int32)}
    try:
        for kw in ({"min_cov": 0}, {"max_ins": 0}, {"max_ins": 65}):
            with pytest.raises(api.HsError, match="out of range"):
                api.polish_haplotypes(batch, sr, polish_everything=True, params=api.consensus_params(**kw))
            with pytest.raises(api.HsError, match="out of range"):
                api.polish_consensus(cc.pack(cc.trim_cases()), api.consensus_params(**kw), form="planned")
        with pytest.raises(api.HsError, match="bad arguments"):
            api.polish_haplotypes(batch, sr, polish_everything=True, c0=1, c1=0)
        bad = cc.pack(cc.trim_cases())
        bad["piece_sam_pos"] = np.zeros_like(bad["piece_sam_pos"])
        with pytest.raises(api.HsError, match="start position"):
            api.polish_consensus(bad, form="planned")
        whole = api.polish_haplotypes(batch, sr, polish_everything=True)
        assert whole["n_bundles"] == 1 and len(api.haplotype_text(whole, 0)) > 19_000
        monkeypatch.setenv("HS_CONSENSUS_CHUNK_MB", "1")
        with pytest.raises(api.HsError, match=r"bundle 0 alone takes \d+ row bytes, more than HS_CONSENSUS_CHUNK_MB allows"):
            api.polish_haplotypes(batch, sr, polish_everything=True)
        big = cc.pack([cc.Bundle("small", cc.BB, [(1, "10M", cc.BB)] * 3), cc.Bundle("big", cc.seq(7000, 1), [(1, "7000M", cc.seq(7000, 1))] * 160)])
        with pytest.raises(api.HsError, match=r"bundle 1 alone takes 1120000 row bytes"):
            api.polish_consensus(big, form="planned")
    finally:
        batch.close()


# ---- 7. the limits -------------------------------------------------------------------------------------------------------------------------
FORMS = ("host", "device", "planned")


@pytest.mark.parametrize("group", sorted(hc.LIMIT_CASES))
def test_limit_cases_agree_on_the_three_routes_and_the_device_plan_equals_the_run_length_plan(built, group):
    """where every case aims is its `aim` (tests/haplotype_cases.py), and the assertion messages carry it"""
    from hairsplitter_amd import api
    bundles = hc.LIMIT_CASES[group]()
    job = cc.pack(bundles)
    aims = [(b.name, b.aim) for b in bundles]
    want_plan, _ = hc.piece_plan_rl(job)
    hc.check_limit_plan(bundles, want_plan)
    for params in ((cc.MIN_COV, cc.MAX_INS), (1, 2), (4, 64)):
        prm = api.consensus_params(min_cov=params[0], max_ins=params[1])
        want = cc.rule_rl(job, *params)
        res = {"host": api.polish_consensus(job, prm, form="host")}
        for run in (0, 1):      # (twice: nothing may hinge on the order in which the pieces' additions arrive)
            res.update({form: api.polish_consensus(job, prm, form=form) for form in FORMS[1:]})
            for form in FORMS:
                cc.assert_same(cc.result_as_rule(res[form]), want, (group, params, run, form, aims))
            _same(res["device"], res["host"], (group, params, run, aims))
            _same(res["planned"], res["host"], (group, params, run, aims))
            assert np.array_equal(res["planned"]["plan"], want_plan), (group, params, run, aims, res["planned"]["plan"].tolist())
            hc.check_limit_plan(bundles, res["planned"]["plan"])
        if params == (cc.MIN_COV, cc.MAX_INS):
            for form in FORMS:
                cc.check_claims(bundles, cc.result_as_rule(res[form]))


@pytest.mark.parametrize("case", range(len(hc.refused_cases())))
def test_a_cigar_over_the_limit_is_refused_on_the_three_routes_naming_the_same_bundle(built, case):
    """refused, not skipped: by the host half, by the host's plan (hs_capi_consensus.inc, consensus_device) and from the device's first_long, an
    atomic minimum over the pieces -- twice, for the order in which two long pieces arrive there"""
    from hairsplitter_amd import api
    name, bundles, named = hc.refused_cases()[case]
    job = cc.pack(bundles)
    for run in (0, 1):
        for form in FORMS:
            with pytest.raises(api.HsError, match=r"bundle %d: a CIGAR of more than 2\^31 - 1 bases" % named):
                api.polish_consensus(job, form=form)


# ---- 6. the default step -------------------------------------------------------------------------------------------------------------------
def test_default_step_costs_what_it_cost_before_a_haplotype_call(built):
    from hairsplitter_amd import api
    from test_gpu_alleles import _job
    from test_gpu_recruit import _step_cost
    pg = api.PipelineGroups(_job(), 2)
    try:
        before = _step_cost(pg, api)
        n = pg.flat.n_contigs
        sr = {"win_off": np.zeros(n + 1, np.int64), "win_start": np.zeros(0, np.int32), "win_end": np.zeros(0, np.int32), "label_off": np.zeros(1, np.int64),
              "labels": np.zeros(0, np.int32)}
        hap = api.polish_haplotypes(pg, sr, polish_everything=True)
        assert 1 <= hap["n_bundles"] <= n and hap["n_pieces"] > 0      # (a contig without reads has no bundle)
        assert _step_cost(pg, api) == before
    finally:
        pg.close()
