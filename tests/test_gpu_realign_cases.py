"""k_realign_cut, k_anchor_join_plan and k_anchor_join on the device through their taps (api.realign_cut_tap, api.anchor_join_tap: the job's own launches)
against the restatements of tests/realign_cases.py, whole buffers by np.array_equal, guard bytes behind them included; the refusals of both taps; and the
jobs whose piece classes sit on the section seams of realign_job, through hs_realign_intervals_anchored against the stitched expectation.
tests/test_cpu_realign_cases.py proves without a GPU that the restatements hold and that every case reaches the forks it names."""
import re

import numpy as np
import pytest

import anchor_cases as ac
import realign_cases as rc

pytestmark = pytest.mark.gpu
PAD = 100
GUARD = 64


def _cut_equals(api, c, fill):
    want = rc.cut(c["seq"], c["off"], c["src"], c["rev"])
    got = api.realign_cut_tap(c["seq"], c["off"], c["src"], c["rev"], fill=fill)
    assert len(got) == len(want) + GUARD
    assert np.array_equal(got[:len(want)], want), np.flatnonzero(got[:len(want)] != want)[:8]
    assert (got[len(want):] == fill).all()


@pytest.mark.parametrize("name", sorted(rc.CUT_CASES))
def test_cut(built, name):
    """the whole output of k_realign_cut, the zeros behind off[m] and the guard bytes behind those; twice in one layout, once with the pieces in another order"""
    from hairsplitter_amd import api
    c = rc.CUT_CASES[name]
    _cut_equals(api, c, 0xA5)
    _cut_equals(api, c, 0x00 if name.startswith("all_bytes") else 0x5A)
    _cut_equals(api, rc.cut_reordered(c, np.random.default_rng(len(c["src"])).permutation(len(c["src"]))), 0xA5)


def _join_equals(api, t, fill):
    plan = rc.join_plan(t)
    want = rc.join(t, plan)
    got = api.anchor_join_tap(t, fill=fill)
    for f in ("pc_at", "out_len", "out_dist", "out_pos"):
        assert np.array_equal(got[f], plan[f]), (f, np.flatnonzero(got[f] != plan[f])[:8])
    assert len(got["joined"]) == len(want) + GUARD
    assert np.array_equal(got["joined"][:len(want)], want), np.flatnonzero(got["joined"][:len(want)] != want)[:8]
    assert (got["joined"][len(want):] == fill).all()
    return got


@pytest.mark.parametrize("name", sorted(rc.JOIN_CASES))
def test_join(built, name):
    """what k_anchor_join_plan leaves and the whole joined buffer of k_anchor_join: the moves themselves ('=' and X apart), the zeros behind every interval's
    moves and behind join_off[m], the guard bytes; twice in one layout, once with the intervals in another order and the moves at other places"""
    from hairsplitter_amd import api
    t = rc.join_case(name)
    _join_equals(api, t, 0xA5)
    got = _join_equals(api, t, 0x5A)
    _join_equals(api, rc.join_case(name, True), 0xA5)
    if name.startswith("dropped"):
        drop = np.flatnonzero(got["out_len"] < 0)
        assert drop.tolist() == [0, 2, 4] and (got["out_dist"][drop] == -1).all() and (got["out_pos"][drop] == -1).all()
        for k in drop:
            assert not got["joined"][t["join_off"][k]:t["join_off"][k + 1]].any()


def test_refused_tables_launch_nothing(built):
    """every host check of the two taps, a step outside: the stated message, and no wait for the device (a tap that had launched would have to wait for
    its download)"""
    from hairsplitter_amd import api
    good, bad = rc.cut_refused()
    api.realign_cut_tap(good["seq"], good["off"], good["src"], good["rev"])
    for name, a, _, msg in bad:
        n0 = api.host_waits()
        with pytest.raises(api.HsError, match=re.escape(msg)):
            api.realign_cut_tap(a["seq"], a["off"], a["src"], a["rev"], out_cap=a.get("out_cap"), m=a.get("m"))
        assert api.host_waits() == n0, name
    good, bad = rc.join_refused()
    api.anchor_join_tap(good)
    for name, t, cap, msg in bad:
        n0 = api.host_waits()
        with pytest.raises(api.HsError, match=re.escape(msg)):
            api.anchor_join_tap(t, joined_cap=cap)
        assert api.host_waits() == n0, name


def _pairs_seam_job(n_iv):
    """one contig, n_iv error-free reads of 10 000 bases but for a few substitutions, anchors at q = 0 .. 9998 on the true diagonal: no head, 9 998 middles
    of one base against one base and a tail of two bases, 10 000 pairs an interval as realign_job counts them (anchors + 1)"""
    g = np.random.default_rng([0x5053, 1])
    L, step = 10000, 13
    C = g.integers(0, 4, size=L + step * 101 + 300).astype(np.uint8)
    reads, ivs, subs = [], [], []
    for i in range(n_iv):
        s = 50 + step * i
        r = C[s:s + L].copy()
        at = g.choice(L - 2, size=1 + i % 4, replace=False)      # (inside the middles)
        r[at] = (r[at] + 1 + g.integers(0, 3, size=len(at))) & 3
        strand = i & 1
        reads.append(r if strand else (3 - r[::-1]).astype(np.uint8))
        ivs.append((i, 0, strand, 0, L, s, s + L))
        subs.append(len(at))
    q = np.tile(np.arange(L - 1, dtype=np.int32), n_iv)
    t = q + np.repeat(np.array([iv[5] for iv in ivs], np.int32), L - 1)
    flat = dict(contig_seq=C, contig_off=np.array([0, len(C)], np.int64), read_seq=np.concatenate(reads), read_off=np.arange(n_iv + 1, dtype=np.int64) * L)
    return flat, np.array(ivs, np.int64), np.arange(n_iv + 1, dtype=np.int64) * (L - 1), q, t, subs


def test_round_seam_on_pairs(built):
    """realign_job closes a round when the next interval's pairs would pass a million: 100 intervals of 10 000 pairs are one round, 101 are two. Every record
    is one M word of 10 000, pos = tstart, NM = its substitutions (no aligner needed to say so); the first 100 are equal in both jobs."""
    import time
    from hairsplitter_amd import api
    recs = []
    for n_iv in (100, 101):
        flat, ivs, off, q, t, subs = _pairs_seam_job(n_iv)
        t0 = time.perf_counter()
        rec, _ = api.realign_intervals_anchored(flat, ivs, off, q, t, pad=PAD, want_batch=False)
        print("pairs seam: %d intervals, %d pieces, %d rounds, %.2f s" % (n_iv, rec["n_pieces"], rec["n_rounds"], time.perf_counter() - t0))
        assert rec["n_rounds"] == (1 if n_iv == 100 else 2) and rec["n_dropped"] == 0 and rec["n_pieces"] == n_iv * 9999
        got = _records(rec)
        assert sorted(got) == list(range(n_iv))
        for i in range(n_iv):
            pos, nm, strand, words = got[i]
            assert (pos, nm, strand, words.tolist()) == (int(ivs[i][5]), subs[i], i & 1, [10000 << 4]), (i, got[i])
        recs.append(got)
    assert all(recs[0][i][:3] == recs[1][i][:3] and np.array_equal(recs[0][i][3], recs[1][i][3]) for i in range(100))


def _records(rec):
    return {int(i): (int(rec["rec_pos"][k]), int(rec["rec_dist"][k]), int(rec["rec_strand"][k]), rec["cigar"][rec["rec_cig_off"][k]:rec["rec_cig_off"][k + 1]])
            for k, i in enumerate(rec["rec_interval"])}


@pytest.mark.parametrize("name", sorted(rc.ROUTE_CASES))
def test_class_sections(built, name):
    """one-round jobs whose HW, SHW and NW classes hold 63, 64 and 65 pieces in three rotations (the numbers of a class begin at a multiple of 64, its
    moves at a multiple of 256), and a job without an HW piece: words, pos, NM, strand and n_pieces equal the stitched pieces'"""
    from hairsplitter_amd import api
    job = rc.route_job(name)
    assert rc.route_classes(job, PAD) == rc.ROUTE_CASES[name]
    rec, _ = api.realign_intervals_anchored(job["flat"], job["ivs"], job["off"], job["aq"], job["at"], pad=PAD, want_batch=False)
    want = ac.expected_records(api, job, PAD)
    got = _records(rec)
    assert rec["n_rounds"] == 1 and rec["n_dropped"] == 0 and sorted(got) == list(range(len(job["ivs"])))
    for i, w in enumerate(want):
        pos, nm, strand, words = got[i]
        assert (pos, nm, strand) == (w["pos"], w["nm"], int(job["ivs"][i][2])) and np.array_equal(words, w["words"]), (i, got[i], w)
    assert rec["n_pieces"] == sum(w["n_pieces"] for w in want) == sum(rc.ROUTE_CASES[name])
