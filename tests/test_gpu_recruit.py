"""The recruit table on the device (hs_kernels_recruit.hip through hs_recruit_reads, hs_group_recruit, HS_PIPELINE_RECRUIT and HS_RECRUIT=1) against the
brute-force statement of the rule in tests/recruit_cases.py, by integer equality of every field. tests/test_cpu_recruit_cases.py proves that every case
reaches the fork it is named after."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

import allele_cases as ac
import golden_util as gu
import recruit_cases as rc
from test_cpu_recruit_cases import RUNS
from test_gpu_alleles import _col_and_gro, _group_columns, _job

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5


@pytest.fixture(scope="module")
def brute():
    """the rule's table of every (case, params), computed once"""
    out = {}
    for name, i in RUNS:
        ctgs, sr, prms = rc.get(name)
        out[(name, i)] = (ctgs, sr, prms[i], rc.recruit_brute(ctgs, sr, prms[i]))
    return out


@pytest.mark.parametrize("name,i", RUNS)
def test_device_table_equals_the_rule(built, brute, name, i):
    """depth: columns of 1 .. 4097 entries, of rows only, of none, empty; groups: 0 .. 300 groups (one lane per row up to 64, one wavefront beyond); which:
    every bit; rule: every branch of the choice and of (a), (b), (c); windows: borders, empty windows and contigs, indices outside the contig's reads"""
    from hairsplitter_amd import api
    ctgs, sr, prm, want = brute[(name, i)]
    got, alleles = api.recruit_reads(ctgs, sr, prm, with_alleles=True)
    assert rc.differences(want, got) == []
    assert got["n_assigned"] == int((want["rows"]["assigned"] != 0).sum()) and got["params"] == prm
    assert got["n_counter_words"] == int((1 + 2 * want["row_groups"]).sum())
    assert ac.differences(api.haplotype_alleles(ctgs, sr), alleles) == []      # the allele table returned alongside
    assert np.array_equal(api.recruit_apply(got, sr), rc.apply_numpy(want, sr))
    assert api.recruit_text(got, ["c%d" % c for c in range(len(ctgs))]) == rc.text(want, ["c%d" % c for c in range(len(ctgs))])


@pytest.mark.parametrize("name,i", [("depth", 0), ("groups", 0), ("rule", 0), ("which", 3), ("windows", 0), ("empty", 0)])
def test_kernel_level_call_in_its_two_steps(built, brute, name, i):
    """hs_group_recruit on device pointers over a work buffer and a row buffer filled with a byte: the rows of the plan are the table's, the row offsets
    cover every window of the call, nothing lies behind the counted rows or between the parts of the work buffer"""
    from hairsplitter_amd import api
    ctgs, sr, prm, want = brute[(name, i)]
    got = api.group_recruit(ctgs, sr, prm, fill=FILL, extra_rows=7)
    assert got["status"] == 0
    assert np.array_equal(got["rows"].astype(rc.ROW), want["rows"])
    assert len(got["rows_tail"]) == 7 * rc.ROW.itemsize + 8 and np.all(got["rows_tail"] == FILL)
    assert got["work_gaps_untouched"]
    per_window = np.zeros(len(sr["win_start"]), np.int64)
    per_window[want["win_index"]] = np.diff(want["win_row_off"])
    assert np.array_equal(got["win_row_off"], np.concatenate(([0], np.cumsum(per_window))))
    assert int(got["flag"].sum()) == len(want["rows"]) and set(np.unique(got["flag"]).tolist()) <= {0, 1}
    assert got["n_counter_words"] == int((1 + 2 * want["row_groups"]).sum())
    has = got["win_snp_last"] > got["win_snp_first"]
    assert np.array_equal(np.flatnonzero(has), want["win_index"])


@pytest.mark.parametrize("bad", rc.REFUSED)
def test_refused_thresholds_leave_no_table(built, bad):
    from hairsplitter_amd import api
    lib = api.load()
    ctgs, sr, _ = rc.get("rule")
    with pytest.raises(api.HsError):
        api.recruit_reads(ctgs, sr, rc.params(**bad))
    arr, keep = api._sr_contig_array(ctgs)
    keep2 = []
    r = api._sr_struct(sr, len(ctgs), keep2)
    prm = api.RecruitParams(*[rc.params(**bad)[k] for k in api.RECRUIT_PARAM_KEYS])
    rt, at = C.POINTER(api.RecruitTable)(), C.POINTER(api.AlleleTable)()
    assert lib.hs_recruit_reads(arr, C.c_int32(len(ctgs)), C.byref(r), C.byref(prm), C.byref(at), C.byref(rt)) == -2      # HS_EINVAL
    assert not rt and not at
    pg = api.PipelineGroups(_job()[:1], 1)
    try:
        with pytest.raises(api.HsError):
            pg.recruits(True, rc.params(**bad))
    finally:
        pg.close()


def _stand_alone(pg, sr, labels, prm):
    """the stand-alone call and the numpy rule on the pipeline's own labels and kept columns (HS_PIPELINE_KEEP_COLUMNS must be on for the last call)"""
    from hairsplitter_amd import api
    cols = _group_columns(pg, 0.01)
    n_reads = np.diff(pg.flat.contig_rec_off)
    for c, ctg in enumerate(cols):
        ctg.update(length=int(pg.flat.contig_off[c + 1] - pg.flat.contig_off[c]), read_start=np.zeros(n_reads[c], np.int32), read_end=np.zeros(n_reads[c], np.int32))
    sr_in = {k: sr[k] for k in ("win_off", "win_start", "win_end", "label_off")}
    sr_in["labels"] = labels
    return cols, sr_in, api.recruit_reads(cols, sr_in, prm), rc.recruit_numpy(cols, sr_in, prm)


def test_pipeline_option_gives_the_table_of_the_calls_own_labels(built):
    """HS_PIPELINE_RECRUIT with two contig groups, two-call and fused form, dense and sparse labels, with and without HS_PIPELINE_KEEP_COLUMNS and
    HS_PIPELINE_ALLELES: one table, equal to hs_recruit_reads and to the numpy form on the call's labels and kept columns; labels as with the option off"""
    from hairsplitter_amd import api
    prm = rc.params(which=rc.ABSENT | rc.UNCLUSTERED | rc.LABELLED)
    pg = api.PipelineGroups(_job(), 2)
    try:
        cv0, sr0 = pg.run(0.33, 8)
        labels0 = sr0["labels"].copy()
        assert "recruits" not in sr0
        pg.recruits(True, prm)
        tables = []
        for fused in (False, True):
            cv1, sr1 = pg.run_fused(0.33, 8) if fused else pg.run(0.33, 8)
            assert np.array_equal(sr1["labels"], labels0) and "alleles" not in sr1      # the cells are formed, the allele table is not exposed
            assert cv1["n_columns_downloaded"] == cv0["n_columns_downloaded"]
            tables.append(sr1["recruits"])
        pg.alleles(True)
        pg.keep_columns(True)
        cv2, sr2 = pg.run_fused(0.33, 8)
        tables.append(sr2["recruits"])
        cols, sr_in, alone, want = _stand_alone(pg, sr2, labels0, prm)
        tables.append(alone)
        assert ac.differences(ac.rule_numpy(cols, sr_in), sr2["alleles"]) == []
        pg.sparse_labels(True)
        for fused in (False, True):
            cv3, sr3 = pg.run_fused(0.33, 8) if fused else pg.run(0.33, 8)
            assert sr3["labels"] is None
            tables.append(sr3["recruits"])
        for k, t in enumerate(tables):
            assert rc.differences(want, t) == [], k
            assert t["params"] == prm
        r = want["rows"]
        assert len(r) > 100 and set(want["win_contig"].tolist()) == {0, 3} and (r["assigned"] != 0).any() and (r["label"] == -2).any() and (r["label"] >= 0).any()
        assert want["n_call_windows"] == len(sr2["win_start"]) and np.array_equal(api.recruit_apply(tables[0], sr_in), rc.apply_numpy(want, sr_in))
        pg.recruits(False)
        pg.alleles(False)
        assert "recruits" not in pg.run_fused(0.33, 8)[1]
    finally:
        pg.close()


def _crc(t):
    return zlib.crc32(b"".join(np.ascontiguousarray(t[k]).tobytes() for k in rc.TABLE_KEYS))


_VIA_HOST = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_recruit as t
from hairsplitter_amd import api
pg = api.PipelineGroups(t._job(), 2)
pg.recruits(True)
a = pg.run_fused(0.33, 8)[1]["recruits"]
print("TABLE", len(a["rows"]), t._crc(a))
pg.close()
"""


def test_pipeline_table_is_the_same_with_the_columns_handed_over_through_the_host(built):
    """HS_COLUMNS_VIA_HOST=1 (read once per process: a child): stage 4 uploads the columns itself, the groups' shares come out the same"""
    from hairsplitter_amd import api
    pg = api.PipelineGroups(_job(), 2)
    try:
        pg.recruits(True)
        a = pg.run_fused(0.33, 8)[1]["recruits"]
    finally:
        pg.close()
    want = "TABLE %d %d" % (len(a["rows"]), _crc(a))
    assert len(a["rows"]) > 0
    r = subprocess.run([sys.executable, "-c", _VIA_HOST % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, HS_COLUMNS_VIA_HOST="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and want in r.stdout.decode().splitlines(), r.stdout.decode()[-2000:]


def _step_cost(pg, api):
    """host waits and kernel launches (by family) of one fused step. Five steps, the fewest waits: a wait that finds its work done already is not
    counted (stream_wait_quiet), so a slow step can count one that a fast step does not."""
    api.kernel_stats_every(1)
    pg.run_fused(0.33, 8)      # (the first step of a pipeline sizes its buffers)
    waits = []
    for _ in range(5):
        api.kernel_stats_reset()
        w0 = api.host_waits()
        pg.run_fused(0.33, 8)
        waits.append(api.host_waits() - w0)
    return min(waits), {k: v["launches"] for k, v in api.kernel_stats().items()}


def test_option_off_costs_what_a_pipeline_that_never_had_it_costs(built):
    """no launch and no host wait stays behind when the option is switched off again; switched on, the step makes the allele route's two waits more,
    not three, and with HS_PIPELINE_ALLELES as well no more than that"""
    from hairsplitter_amd import api
    fresh = api.PipelineGroups(_job(), 2)
    try:
        base = _step_cost(fresh, api)
    finally:
        fresh.close()
    pg = api.PipelineGroups(_job(), 2)
    try:
        pg.alleles(True)
        with_alleles = _step_cost(pg, api)
        pg.recruits(True)
        both = _step_cost(pg, api)
        pg.alleles(False)
        recruit_only = _step_cost(pg, api)
        pg.recruits(False)
        off = _step_cost(pg, api)
    finally:
        pg.close()
    assert off == base
    assert both[0] == with_alleles[0] == recruit_only[0] > base[0]
    assert both[1]["other"] > with_alleles[1]["other"] > base[1].get("other", 0) and recruit_only[1] == both[1]
    assert {k: v for k, v in both[1].items() if k != "other"} == {k: v for k, v in base[1].items() if k != "other"}


def test_executable_writes_the_table_of_its_own_run(built):
    """HS_RECRUIT=1: <outfile> is byte-identical with and without it (and the precomputed .gro is not adopted), <outfile>.recruit.tsv is the text of the rule's
    table on the .gro's labels and the .col's columns, <outfile>.recruited.gro what the writer makes of the applied labels; without the variable no such files"""
    from hairsplitter_amd import api
    with tempfile.TemporaryDirectory() as td:
        meta = gu.unpack("multi", td)
        env = dict(os.environ, HS_NO_DETACH="1")
        env.pop("HS_RECRUIT", None)
        col = os.path.join(td, "variants.col")
        er = meta["error_rate_arg"]

        def stage4(out, env):
            r = subprocess.run([built["sr"], col, "1", er, os.path.join(td, "no_ploidy"), "0", "0.01", "0", os.path.join(td, out), "0"],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
            assert r.returncode == 0, r.stdout.decode()[-2000:]
            return open(os.path.join(td, out), "rb").read()

        plain = stage4("a.gro", env)
        with_table = stage4("b.gro", dict(env, HS_RECRUIT="1"))
        assert plain == with_table and len(plain) > 0
        assert not os.path.exists(os.path.join(td, "a.gro.recruit.tsv")) and not os.path.exists(os.path.join(td, "a.gro.recruited.gro"))
        assert not os.path.exists(os.path.join(td, "b.gro.alleles.tsv"))
        text = open(os.path.join(td, "b.gro.recruit.tsv")).read()
        names, contigs, sr = _col_and_gro(col, os.path.join(td, "b.gro"), 0.01)
        want = rc.recruit_numpy(contigs, sr, rc.DEFAULT)
        assert text == rc.text(want, names) and text.count("WINDOW\t") == len(want["win_start"]) > 0 and text.count("READ\t") == len(want["rows"]) > 0
        assert (want["rows"]["assigned"] != 0).any()
        # the .recruited.gro: the .gro of the applied labels -- parsed back, its labels are hs_recruit_apply's
        _, _, sr_applied = _col_and_gro(col, os.path.join(td, "b.gro.recruited.gro"), 0.01)
        applied = rc.apply_numpy(want, sr)
        assert np.array_equal(sr_applied["labels"], applied) and (applied != sr["labels"]).any()
        assert np.array_equal(api.recruit_apply(api.recruit_reads(contigs, sr), sr), applied)
        # and byte for byte what the writer gives on them: every GROUP line lists the reads whose applied label is not -2
        lines = [l for l in open(os.path.join(td, "b.gro.recruited.gro")).read().split("\n") if l.startswith("GROUP\t")]
        k = 0
        for c in range(len(contigs)):
            if len(contigs[c]["snp_pos"]) == 0:
                continue      # (the writer skips contigs without SNPs, separate_reads.cpp:1522-1524)
            for w in range(int(sr["win_off"][c]), int(sr["win_off"][c + 1])):
                lab = applied[int(sr["label_off"][w]):int(sr["label_off"][w + 1])]
                ids = np.flatnonzero(lab != -2)
                assert lines[k] == "GROUP\t%d\t%d\t%s\t%s" % (sr["win_start"][w], sr["win_end"][w], "".join("%d," % i for i in ids), "".join("%d," % lab[i] for i in ids)), (c, w)
                k += 1
        assert k == len(lines)
        other = [l for l in open(os.path.join(td, "b.gro.recruited.gro")).read().split("\n") if not l.startswith("GROUP\t")]
        assert other == [l for l in plain.decode().split("\n") if not l.startswith("GROUP\t")]
