"""The haplotype route without a device: (a) on every case of tests/haplotype_cases.py the C++ host half (hs_polish_consensus_host,
through tests/harness/consensus_selftest) equals the numpy form of tests/consensus_cases.py, and every claim holds -- the cases are ones the
reference half already handles; (b) the numpy restatement of the plan of a piece agrees with that form's n_skipped and record count on every
case of both files, and piece by piece with hs::cons_piece_plan (tests/harness/haplotypes_selftest); (c) the FASTA record as a device-free
function; (d) the header declares what the binding binds. The selftest runs once under its AddressSanitizer build."""
import os
import re
import subprocess

import numpy as np
import pytest

import consensus_cases as cc
import haplotype_cases as hc
from test_cpu_consensus import run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")
GROUPS = dict(hc.all_groups())


@pytest.fixture(scope="module")
def consensus_selftest(built):
    return os.path.join(HARNESS, "_build", "consensus_selftest")


@pytest.fixture(scope="module")
def selftest(built):
    return built["haplotypes_selftest"]


def run_lines(exe, lines, tmp_path):
    path = str(tmp_path / "lines.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode()


@pytest.mark.parametrize("group", sorted(hc.CASES))
def test_host_half_equals_the_numpy_form_on_the_new_cases(consensus_selftest, tmp_path, group):
    bundles = hc.CASES[group]()
    job = cc.pack(bundles)
    want = cc.rule(job)
    cc.check_claims(bundles, want)
    got = run_host(consensus_selftest, job, tmp_path)
    cc.assert_same(got, want, group)
    cc.check_claims(bundles, got)


def plan_lines(job, bundle):
    out = []
    for p in range(len(bundle)):
        b = int(bundle[p])
        w = job["cigar"][job["cig_off"][p]:job["cig_off"][p + 1]]
        out.append("P %d %d %d %d %d %s" % (job["base_off"][p + 1] - job["base_off"][p], job["piece_flags"][p], job["piece_sam_pos"][p],
                                           job["backbone_off"][b + 1] - job["backbone_off"][b], len(w), " ".join(str(int(x)) for x in w)))
    return out


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_the_restated_plan_agrees_with_the_rule_and_with_the_host(selftest, tmp_path, group):
    job = cc.pack(GROUPS[group])
    want = cc.rule(job)
    plan, bundle = hc.piece_plan(job)
    nb = len(job["backbone_off"]) - 1
    assert np.bincount(bundle[plan[:, 0] == 1], minlength=nb).tolist() == want["n_skipped"]
    assert int(plan[:, 3].sum()) == want["n_ins_records"]
    assert not plan[:, 1].any()
    if len(bundle):
        got = [[int(x) for x in line.split()[1:]] for line in run_lines(selftest, plan_lines(job, bundle), tmp_path).splitlines()]
        assert got == plan.tolist()


def test_the_new_cases_reach_what_they_name():
    """a voting insertion at each chunk edge, a clipped room, a skipped 130-op piece: read off the restated plan, so that a case that lost its
    shape through an edit fails here"""
    plans = {g: hc.piece_plan(cc.pack(hc.CASES[g]()))[0] for g in hc.CASES}
    assert plans["chunk_edges"][::3, 3].tolist() == [1, 1, 1, 1, 0] and plans["chunk_edges"][::3, 2].tolist() == [68, 132, 68, 66, 10]
    assert plans["room"][::3].tolist() == [[0, 0, 40, 0], [0, 0, 40, 1], [0, 0, 80, 10]]
    assert plans["skip"][:, 0].tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert [len(plans["count%d" % n]) for n in (0, 1, 4, 5)] == [0, 1, 4, 5]
    for g in ("chunk_edges", "room", "skip"):
        assert max(len(p[1]) for b in hc.CASES[g]() for p in b.pieces) > 64


# ---- the run-length restatements, and the limit cases they exist for ------------------------------------------------------------------------
def _old_groups():
    import refine_cases as rc
    return hc.all_groups() + [("rc." + g, rc.CASES[g]()) for g in sorted(rc.CASES)]


@pytest.mark.parametrize("params", ((cc.MIN_COV, cc.MAX_INS), (1, 2), (4, 64)))
def test_run_length_forms_equal_the_expanding_forms_on_every_old_group(params):
    """cc.rule_rl, hc.piece_plan_rl and rc.columns_rl against the forms that hold one array entry per event, in every field"""
    import refine_cases as rc
    for name, bundles in _old_groups():
        job = cc.pack(bundles)
        a, b = cc.rule(job, *params), cc.rule_rl(job, *params)
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k] == b[k], (name, params, k)
        for x, y in zip(hc.piece_plan(job), hc.piece_plan_rl(job)):
            assert np.array_equal(x, y), (name, "plan")
        for k, x, y in zip(("col_off", "col_begin", "col_ins"), rc.columns(job, *params), rc.columns_rl(job, *params)):
            assert x.dtype == y.dtype and np.array_equal(x, y), (name, params, k)


@pytest.mark.parametrize("group", sorted(hc.LIMIT_CASES))
def test_host_half_and_host_plan_equal_the_run_length_forms_on_the_limit_cases(consensus_selftest, selftest, tmp_path, group):
    """the builders assert their sums (T, Q, T + Q) as they build; the claims and the claimed plans are worked out by hand"""
    bundles = hc.LIMIT_CASES[group]()
    job = cc.pack(bundles)
    plan, bundle = hc.piece_plan_rl(job)
    hc.check_limit_plan(bundles, plan)
    got = [[int(x) for x in line.split()[1:]] for line in run_lines(selftest, plan_lines(job, bundle), tmp_path).splitlines()]
    assert got == plan.tolist()
    for params in ((cc.MIN_COV, cc.MAX_INS), (1, 2), (4, 64)):
        want = cc.rule_rl(job, *params)
        assert np.bincount(bundle[plan[:, 0] == 1], minlength=len(bundles)).tolist() == want["n_skipped"] and int(plan[:, 3].sum()) == want["n_ins_records"]
        res = run_host(consensus_selftest, job, tmp_path, *params)
        cc.assert_same(res, want, (group, params))
        if params == (cc.MIN_COV, cc.MAX_INS):
            cc.check_claims(bundles, want)
            cc.check_claims(bundles, res)


def test_the_limit_cases_reach_what_they_name():
    sums = {b.name: b.sums for g in hc.LIMIT_CASES for b in hc.LIMIT_CASES[g]()}
    assert sum(sums["at the limit: 5M, 7 x 268435455D, 268435452D"]) == hc.INT32_MAX == sum(sums["at the limit, M and I form: 4 x 268435455M 3M 1I"])
    assert sums["full chunk: 5M and 63 x 33554432D"][0] == 63 * 2 ** 25 + 5 < 2 ** 31
    for b in hc.LIMIT_CASES["long_m"]():
        assert 2 ** 16 < len(b.backbone) <= 70_000 and len(b.pieces) == 3
    assert all(len(b.backbone) <= 100 and len(b.pieces) <= 4 for g in ("lengths", "chunks", "boundary") for b in hc.LIMIT_CASES[g]())
    assert len(hc.LIMIT_CASES["chunks"]()[0].pieces[0][1]) == 64 == len(hc.LIMIT_CASES["chunks"]()[1].pieces[0][1])
    assert sum(sums["at the limit, a full chunk: 5M, 62 x 33554432D, 67108853D"]) == hc.INT32_MAX and len(hc.FULL_AT_LIMIT) == 64 == len(hc.FULL_OVER_LIMIT)


@pytest.mark.parametrize("case", range(len(hc.refused_cases())))
def test_a_cigar_over_the_limit_is_refused_by_the_host_half_and_flagged_by_the_host_plan(consensus_selftest, selftest, tmp_path, case):
    name, bundles, named = hc.refused_cases()[case]
    job = cc.pack(bundles)
    plan, bundle = hc.piece_plan_rl(job)
    assert plan[:, 1].any() and int(bundle[plan[:, 1] == 1].min()) == named, name
    got = [[int(x) for x in line.split()[1:]] for line in run_lines(selftest, plan_lines(job, bundle), tmp_path).splitlines()]
    assert got == plan.tolist(), name
    path = str(tmp_path / "job.txt")
    for threads in (1, 2):
        cc.write_job(path, job, threads=threads)
        r = subprocess.run([consensus_selftest, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 4 and r.stdout == b"", (name, r.returncode)
        assert r.stderr.decode() == "consensus_selftest: bundle %d: a CIGAR of more than 2^31 - 1 bases\n" % named, (name, r.stderr.decode())


FASTA_LINES = ["F contig_1 100 2099 0 3 7 ACGTACGTAC", "F edge_7 0 500 -1 0 4 ACGT", "F c 5 6 2 4 4 ACGTACGT", "F c 5 6 3 0 0 -", "F c 1 2 12 6 2 ACGTACGT"]
FASTA_WANT = ">contig_1_100_2099_0\nTACG\n>edge_7_0_500_-1\nACGT\n>c_5_6_2\n\n>c_5_6_3\n\n>c_1_2_12\n\n"


def test_fasta_record(selftest, tmp_path):
    """header fields, a group of -1, trim_start = trim_end, an empty consensus, trim_end below trim_start"""
    assert run_lines(selftest, FASTA_LINES, tmp_path) == FASTA_WANT


def test_selftest_under_asan(built, tmp_path):
    subprocess.run(["make", "-s", "-f", "haplotypes_selftest.mk", "asan"], cwd=HARNESS, check=True)
    exe = os.path.join(HARNESS, "_build", "haplotypes_selftest_asan")
    job = cc.pack(hc.chunk_edge_cases() + hc.room_cases() + hc.skip_cases() + cc.edges_cases())
    plan, bundle = hc.piece_plan(job)
    out = run_lines(exe, FASTA_LINES + plan_lines(job, bundle), tmp_path)
    assert out.startswith(FASTA_WANT)
    assert [[int(x) for x in line.split()[1:]] for line in out[len(FASTA_WANT):].splitlines()] == plan.tolist()


def test_header_declares_the_haplotype_symbols():
    from hairsplitter_amd import api
    hdr = open(os.path.join(ROOT, "include", "hairsplitter_hip.h")).read()
    for sym in ("hs_polish_haplotypes", "hs_polish_haplotypes_from_files", "hs_haplotypes_result_destroy", "hs_polish_consensus_planned_tap"):
        assert re.search(r"\b%s\(" % sym, hdr), sym
        assert sym in api.SYMBOLS
    fields = re.search(r"typedef struct hs_haplotypes_result \{(.*?)\} hs_haplotypes_result;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\*?\s*([a-z_]+)\s*[,;]", fields)
    assert names == [n for n, _ in api.HaplotypesResult._fields_], names
