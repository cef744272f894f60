"""tests/realign_cases.py without a GPU: the numpy restatements of k_realign_cut, k_anchor_join_plan and k_anchor_join against plain per-byte loops, the
plan's POS against anchor_cases.stitch (the head placed by its count of non-I moves), per case the forks it claims computed from its layout, and the
refusals of the two taps as predicates over the same tables. tests/test_gpu_realign_cases.py runs the same cases on the device."""
import numpy as np
import pytest

import realign_cases as rc


# ---- the loops: one byte at a time, as the kernels' byte paths read them ----
def cut_loop(seq, off, src, rev):
    out = [0] * rc.round16(off[-1])
    for i in range(len(src)):
        for k in range(int(off[i + 1] - off[i])):
            out[int(off[i]) + k] = (3 - int(seq[int(src[i]) - k])) % 256 if rev is not None and rev[i] else int(seq[int(src[i]) + k])
    return np.array(out, np.uint8)


def join_loop(t):
    m = len(t["iv_base"])
    pc_at, out_len, out_dist, out_pos = [0] * len(t["pc_kind"]), [], [], []
    joined = [0] * rc.round16(t["join_off"][-1])
    for k in range(m):
        p0, p1 = int(t["iv_piece"][k]), int(t["iv_piece"][k + 1])
        at, dist, pos, ok = 0, 0, int(t["iv_base"][k]), p1 > p0
        for p in range(p0, p1):
            kind, i = int(t["pc_kind"][p]), int(t["pc_idx"][p])
            if kind == rc.INS:
                n = i
                dist += n
            else:
                n = int(t["len"][i])
                dist += int(t["dist"][i])
                if kind == rc.HW:
                    pos += int(t["start"][i])
                if kind == rc.HEAD:
                    pos -= int(t["end"][i]) + 1
            ok = ok and 0 < n <= t["pc_room"][p]
            pc_at[p] = at
            at += max(n, 0)
        ok = ok and at <= t["join_off"][k + 1] - t["join_off"][k]
        out_len.append(at if ok else -1); out_dist.append(dist if ok else -1); out_pos.append(pos if ok else -1)
        if not ok:
            continue
        for x in range(at):
            p = max(q for q in range(p0, p1) if pc_at[q] <= x)
            n = (pc_at[p + 1] if p + 1 < p1 else at) - pc_at[p]
            j = x - pc_at[p]
            kind = int(t["pc_kind"][p])
            joined[int(t["join_off"][k]) + x] = 1 if kind == rc.INS else int(t["ops"][int(t["pc_ops"][p]) + (n - 1 - j if kind == rc.HEAD else j)])
    return dict(pc_at=np.array(pc_at, np.int32), out_len=np.array(out_len, np.int32), out_dist=np.array(out_dist, np.int32), out_pos=np.array(out_pos, np.int32)), np.array(joined, np.uint8)


# ---- the cut ----
@pytest.mark.parametrize("name", sorted(rc.CUT_CASES))
def test_cut_restatement_equals_the_loop_and_the_case_reaches_its_forks(name):
    c = rc.CUT_CASES[name]
    want = rc.cut(c["seq"], c["off"], c["src"], c["rev"])
    assert np.array_equal(want, cut_loop(c["seq"], c["off"], c["src"], c["rev"]))
    assert rc.cut_refusal(len(c["seq"]), c["off"], c["src"], c["rev"], out_cap=len(want)) is None
    forks = rc.cut_forks(c)
    assert c["reach"] and set(c["reach"]) <= forks, sorted(set(c["reach"]) - forks)
    order = np.random.default_rng(len(c["src"])).permutation(len(c["src"]))
    s = rc.cut_reordered(c, order)
    assert np.array_equal(rc.cut(s["seq"], s["off"], s["src"], s["rev"]), cut_loop(s["seq"], s["off"], s["src"], s["rev"]))


def test_cut_cases_cover_the_list():
    """every fork the kernel has, somewhere in the cases; a few windows in all"""
    forks = set().union(*(rc.cut_forks(c) for c in rc.CUT_CASES.values()))
    need = ["length %d" % n for n in rc.CUT_LENGTHS] + ["piece begins at %d mod 16" % r for r in range(16)] + ["src %s %d mod 4" % (d, r) for d in ("fwd", "rev") for r in range(4)]
    need += ["block %s sh %d" % (d, r) for d in ("fwd", "rev") for r in range(4)]
    need += ["block a + 16 == off[i + 1]", "bytes a + 16 == off[i + 1] + 1", "bytes 16 pieces", "window > 256 pieces", "bytes fwd | rev", "off[m] % 16 == 0", "off[m] % 16 != 0",
             "off[m] % 4096 == 0", "m == 1", "rev NULL", "rev piece ends on seq[0]", "block rev loads seq[0]", "fwd piece ends on seq[seq_len - 1]", "block fwd loads seq[seq_len - 1]",
             "window p_lo == p_hi", "bytes behind off[m]"]
    assert set(need) <= forks, sorted(set(need) - forks)
    assert any(np.diff(c["off"]).max() > 8192 for c in rc.CUT_CASES.values())
    assert sum(rc.round16(c["off"][-1]) for c in rc.CUT_CASES.values()) <= 16 * 4096


def test_all_byte_values_go_through_both_paths():
    """the 256 byte values, reversed: all of them by whole blocks in one case, all of them byte by byte in the other"""
    for name, whole in (("all_bytes_by_blocks", True), ("all_bytes_by_bytes", False)):
        c = rc.CUT_CASES[name]
        paths = np.repeat(rc.cut_block_paths(c), 16)[:c["off"][-1]]
        values = set()
        for (n, s, r), o in zip(rc.cut_pieces(c), c["off"]):
            if r:
                values |= {int(c["seq"][s - k]) for k in range(n) if paths[o + k] == whole}
        assert values == set(range(256)), name
    want = rc.cut(**{k: rc.CUT_CASES["all_bytes_by_blocks"][k] for k in ("seq", "off", "src", "rev")})
    assert sorted(want[:256].tolist()) == list(range(256)) and want[0] == (3 - 255) % 256


def test_cut_refusals_as_predicates():
    good, bad = rc.cut_refused()
    assert rc.cut_refusal(len(good["seq"]), good["off"], good["src"], good["rev"], out_cap=32) is None
    for name, a, seq_len, msg in bad:
        got = rc.cut_refusal(seq_len, a["off"], a["src"], a["rev"], m=a.get("m"), out_cap=a.get("out_cap"))
        assert got is not None and got.startswith(msg), (name, got, msg)


# ---- the join ----
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("name", sorted(rc.JOIN_CASES))
def test_join_restatement_equals_the_loop_and_the_case_reaches_its_forks(name, shuffled):
    t = rc.join_case(name, shuffled)
    assert rc.join_refusal(t) is None
    plan = rc.join_plan(t)
    want = rc.join(t, plan)
    loop_plan, loop_joined = join_loop(t)
    for f in ("pc_at", "out_len", "out_dist", "out_pos"):
        assert np.array_equal(plan[f], loop_plan[f]), f
    assert np.array_equal(want, loop_joined)
    if not shuffled:
        forks = rc.join_forks(t, plan)
        claimed = rc.JOIN_CASES[name][2]
        assert claimed and set(claimed) <= forks, sorted(set(claimed) - forks)


@pytest.mark.parametrize("name", sorted(rc.JOIN_CASES))
def test_join_plan_equals_the_stitched_record(name):
    """pos, the summed distance (INS runs included) and the joined moves of every kept interval equal anchor_cases.stitch on its pieces; a dropped interval
    has -1 everywhere and no byte"""
    t = rc.join_case(name)
    plan = rc.join_plan(t)
    joined = rc.join(t, plan)
    dropped = 0
    for k, s in enumerate(rc.join_stitched(t)):
        a, b = int(t["join_off"][k]), int(t["join_off"][k + 1])
        if s is None:
            assert (plan["out_len"][k], plan["out_dist"][k], plan["out_pos"][k]) == (-1, -1, -1) and not joined[a:b].any()
            dropped += 1
            continue
        pos, nm, moves = s
        assert (plan["out_pos"][k], plan["out_dist"][k], plan["out_len"][k]) == (pos, nm, len(moves)), (name, k)
        assert np.array_equal(joined[a:a + len(moves)], moves) and not joined[a + len(moves):b].any()
    assert dropped == (3 if name.startswith("dropped") else 0)


def test_join_cases_cover_the_list():
    forks = set()
    for name in rc.JOIN_CASES:
        t = rc.join_case(name)
        forks |= rc.join_forks(t, rc.join_plan(t))
    need = ["block %s" % k for k in rc.KIND_NAME] + ["first piece %s" % k for k in ("HW", "HEAD", "INS", "MID")] + ["block HEAD load at %d mod 4" % r for r in range(4)]
    need += ["%s of %d moves" % (k, n) for k in ("HEAD", "MID", "TAIL") for n in rc.JOIN_LENGTHS]
    need += ["bytes 2 pieces", "bytes >= 3 pieces", "bytes 16 pieces", "bytes 2 intervals with slack", "dropped interval first", "dropped interval middle", "dropped interval last",
             "join_off[m] % 16 == 0", "join_off[m] % 16 != 0", "4096 seam inside a piece", "4096 seam on an interval boundary", "m == 1", "m == 256", "m == 257", "bytes behind join_off[m]"]
    assert set(need) <= forks, sorted(set(need) - forks)


def test_moves_mix_equal_and_mismatch_inside_m_runs():
    """what the words cannot see: inside one M run of a joined string both 0 and 3 occur, so a join that shuffled them would keep every word"""
    t = rc.join_case("kinds_and_lengths")
    joined = rc.join(t, rc.join_plan(t))
    m_run = (joined[:-1] == 0) & (joined[1:] == 3) | (joined[:-1] == 3) & (joined[1:] == 0)
    assert m_run.sum() > 100
    for p, mv in enumerate(t["moves"]):      # the builder's identity: end - start + 1 non-I moves, one edit per move that is not '='
        if mv is not None:
            i = t["pc_idx"][p]
            assert t["end"][i] - t["start"][i] + 1 == (mv != 1).sum() and t["dist"][i] == (mv != 0).sum() and t["len"][i] == len(mv)


def test_join_refusals_as_predicates():
    good, bad = rc.join_refused()
    assert rc.join_refusal(good, joined_cap=rc.round16(good["join_off"][-1])) is None
    for name, t, cap, msg in bad:
        got = rc.join_refusal(t, joined_cap=cap)
        assert got is not None and got.startswith(msg), (name, got, msg)


# ---- the route jobs ----
@pytest.mark.parametrize("name", sorted(rc.ROUTE_CASES))
def test_route_jobs_hold_the_classes_they_name(name):
    job = rc.route_job(name)
    assert rc.route_classes(job, 100) == rc.ROUTE_CASES[name]
    if name == "first_class_empty":
        assert all(len(a) for a in job["ancs"])
