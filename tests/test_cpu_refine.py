"""The device-free half of the polishing passes (hs_refine_host.h), no device: (a) hs_polish_refine_plan_host and the program
tests/harness/refine_selftest equal the numpy restatement of tests/refine_cases.py -- col_begin, col_ins, every window -- on every case, and the hand-worked
windows of the cases hold; (b) the column figures against the EXISTING host half: overhang_left = t gives trim_start == col_begin[t], sum(col_ins) ==
n_ins_bases, the columns that emit nothing are n_del; (c) error-free pieces with nM words are a fixed point; (d) the claims of `scattered` hold through
the host half with a plain Needleman-Wunsch, whichever path it picks; (e) a window rule that includes the slot's insertion changes pass 2 of the case
that claims it; (f) the selftest under its AddressSanitizer build, once."""
import os
import subprocess

import numpy as np
import pytest

import consensus_cases as cc
import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")
SMALL = ("scattered", "window_edges")


@pytest.fixture(scope="module")
def selftest(built):
    return os.path.join(HARNESS, "_build", "refine_selftest")


def host_pass(job, params=None):
    from hairsplitter_amd import api
    return api.polish_refine_plan_host(job, params)


def nw_align(pairs):
    return [rc.nw_moves(q, t) for q, t in pairs]


def run_selftest(exe, job, tmp_path):
    path = str(tmp_path / "job.txt")
    cc.write_job(path, job, threads=2)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    out = cc.parse_selftest(r.stdout.decode())
    begin, ins, ws, we, nxt, sam, word = [], [], [], [], [], [], []
    for line in r.stdout.decode().splitlines():
        f = line.split()
        if f[0] == "K":
            n = int(f[2])
            begin.extend(int(x) for x in f[3:3 + n]); ins.extend(int(x) for x in f[3 + n:3 + 2 * n])
        elif f[0] == "N":
            nxt.append((int(f[2]), int(f[3])))
        elif f[0] == "W":
            ws.append(int(f[2])); we.append(int(f[3])); sam.append(int(f[4])); word.append(int(f[5]))
    out.update({"col_begin": np.array(begin, np.int32), "col_ins": np.array(ins, np.int32), "win_start": np.array(ws, np.int64), "win_end": np.array(we, np.int64),
                "next_overhangs": nxt, "next_sam": sam, "empty_word": word})
    return out


@pytest.mark.parametrize("group", sorted(rc.CASES) + sorted(rc.NOISY))
def test_plan_host_equals_the_restatement(selftest, tmp_path, group):
    bundles = dict(rc.CASES, **rc.NOISY)[group]()
    job = cc.pack(bundles)
    col_off, begin, ins = rc.columns(job)
    ws, we = rc.windows(job, col_off, begin, ins)
    rc.check_windows(bundles, job, ws, we)
    got = host_pass(job)
    want = cc.rule(job)
    for k in cc.FIELDS + ("cons",):
        assert cc.result_as_rule(got)[k] == want[k], (group, k)
    for k, v in (("col_off", col_off), ("col_begin", begin), ("col_ins", ins), ("win_start", ws), ("win_end", we)):
        assert np.array_equal(got[k], v), (group, k)
    rc.check_pass_claims(bundles, 1, got)
    prog = run_selftest(selftest, job, tmp_path)
    for k in cc.FIELDS + ("cons",):
        assert prog[k] == want[k], (group, k)
    for k, v in (("col_begin", begin), ("col_ins", ins), ("win_start", ws), ("win_end", we)):
        assert np.array_equal(prog[k], v), (group, k)
    lens = np.diff(got["cons_off"])
    assert prog["next_overhangs"] == [(int(a), int(n - e)) for a, e, n in zip(got["trim_start"], got["trim_end"], lens)]
    assert prog["next_sam"] == [1 if s < 0 else int(s) + 1 for s in ws]
    n_bases = np.diff(job["base_off"])
    assert prog["empty_word"] == [(int(n) << 4) | 1 if s >= 0 and e == s else 0 for s, e, n in zip(ws, we, n_bases)]


def test_column_figures_against_the_existing_host_half(built):
    from hairsplitter_amd import api
    group = "small"
    job = cc.pack(rc.scattered_cases() + rc.window_edges_cases() + cc.slots_cases() + cc.trim_cases())
    got = host_pass(job)
    L = np.diff(job["backbone_off"])
    for t in range(int(L.max()) + 2):
        probe = dict(job, bundle_overhang_left=np.full(len(L), t, np.int32))
        trim = api.polish_consensus(probe, form="host")["trim_start"]
        for b in range(len(L)):
            assert trim[b] == got["col_begin"][got["col_off"][b] + min(t, int(L[b]))], (group, t, b)
    plain = api.polish_consensus(job, form="host")
    for b in range(len(L)):
        o = int(got["col_off"][b])
        begin, ins = got["col_begin"][o:o + L[b] + 1].astype(np.int64), got["col_ins"][o:o + L[b] + 1].astype(np.int64)
        assert ins.sum() == plain["n_ins_bases"][b] and ins[0] == 0 and ins[L[b]] == 0
        assert int((np.diff(begin) - ins[:L[b]] == 0).sum()) == plain["n_del"][b]
        assert begin[L[b]] == plain["cons_off"][b + 1] - plain["cons_off"][b]
    assert sum(int(x) for x in plain["n_del"]) > 0 and sum(int(x) for x in plain["n_ins_bases"]) > 0


def test_error_free_pieces_are_a_fixed_point(built):
    """full coverage, no error, the words nM supplied here (an alignment of equal strings): pass 2 is pass 1's text and counts nothing"""
    bb = cc.seq(300, 17)
    bundles = [cc.Bundle("error-free", bb, [(1, "300M", bb)] * 3 + [(41, "200M", bb[40:240])] * 2, ovl=20, ovr=30)]
    job = cc.pack(bundles)
    passes = rc.compose(job, 2, host_pass, lambda pairs: [(np.zeros(len(q), np.uint8), 0) for q, t in pairs])
    one, two = passes[0]["res"], passes[1]["res"]
    assert one["cons"].tobytes().decode() == bb and np.array_equal(one["cons"], two["cons"]) and passes[1]["n_pairs"] == 5
    for k in rc.SUMS:
        assert int(two[k].sum()) == 0, k
    assert (int(two["trim_start"][0]), int(two["trim_end"][0])) == (20, 270) == (int(one["trim_start"][0]), int(one["trim_end"][0]))


@pytest.mark.parametrize("group", SMALL)
def test_claims_hold_through_the_host_half_whichever_path_is_picked(built, group):
    bundles = rc.CASES[group]()
    passes = rc.compose(cc.pack(bundles), 3, host_pass, nw_align)
    for p, x in enumerate(passes):
        rc.check_pass_claims(bundles, p + 1, x["res"])
    if group == "scattered":      # pass 1 keeps the backbone's error, pass 2 has the haplotype, pass 3 is a fixed point
        one, two, three = (x["res"] for x in passes)
        assert int(one["n_ins_bases"][0]) == 0 and int(two["n_ins_bases"][0]) == 2 and np.array_equal(two["cons"], three["cons"])
        assert all(int(three[k].sum()) == 0 for k in rc.SUMS)


def test_a_window_that_includes_the_slots_insertion_changes_pass_two(built):
    b = rc.slot_in_front_case()
    job = cc.pack([b])
    one = host_pass(job)
    col_off, begin, ins = rc.columns(job)
    ws, we = rc.windows(job, col_off, begin, ins)
    bad_ws, bad_we = rc.windows(job, col_off, begin, ins, include_slot=True)
    rc.check_windows([b], job, ws, we)
    rc.check_windows([b], job, bad_ws, bad_we, key="wrong_windows")
    right = host_pass(rc.next_job(job, one, ws, we, nw_align)[0])
    wrong = host_pass(rc.next_job(job, one, bad_ws, bad_we, nw_align)[0])
    rc.check_pass_claims([b], 2, right)
    assert wrong["cons"].tobytes().decode() == b.claim["wrong_pass2"]["cons"] != right["cons"].tobytes().decode()
    assert int(wrong["n_del"][0]) == b.claim["wrong_pass2"]["n_del"] and int(right["n_del"][0]) == 0


def test_refused_parameters_and_arrays(built):
    from hairsplitter_amd import api
    job = cc.pack(rc.scattered_cases())
    for kw in ({"min_cov": 0}, {"max_ins": 65}):
        with pytest.raises(api.HsError, match="out of range"):
            api.polish_refine_plan_host(job, api.consensus_params(**kw))
    with pytest.raises(api.HsError, match="start position"):
        api.polish_refine_plan_host(dict(job, piece_sam_pos=np.zeros_like(job["piece_sam_pos"])))


def test_selftest_under_asan(built, tmp_path):
    subprocess.run(["make", "-s", "-f", "refine_selftest.mk", "asan"], cwd=HARNESS, check=True)
    bundles = rc.scattered_cases() + rc.window_edges_cases() + cc.slots_cases() + cc.pieces_cases()
    job = cc.pack(bundles)
    got = run_selftest(os.path.join(HARNESS, "_build", "refine_selftest_asan"), job, tmp_path)
    col_off, begin, ins = rc.columns(job)
    ws, we = rc.windows(job, col_off, begin, ins)
    for k, v in (("col_begin", begin), ("col_ins", ins), ("win_start", ws), ("win_end", we)):
        assert np.array_equal(got[k], v), k
    for k in cc.FIELDS + ("cons",):
        assert got[k] == cc.rule(job)[k], k
