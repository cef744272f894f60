"""The cases of tests/loop_a_cases.py are what their table says, and the host form of loop A equals the oracle on them: no GPU. Every claim is proven
with the oracle's per-column tap (oracle_lib.loop_a: the fate of every column, every (column, partition) pair the loop met with its 2x2 table, second
allele and verdicts). loop_a_cases.restate is loop A restated in numpy with the books of the device form's limits on the side; it must reproduce the
oracle before its verdicts (on_device, failed, reason) are believed, and its wrong forms (other tie rules, last_position moved on create) must give
other partitions. tests/harness/host_harness loop_a (hs::cv_build_cand_bits -> hs::cv_phase_a_host under -DHS_SELFCHECK -> the dense export) is
compared with the oracle by integer equality."""
import os
import subprocess

import numpy as np
import pytest

import loop_a_cases as lc
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "_build", "host_harness")


@pytest.fixture(scope="module", autouse=True)
def _artefacts(built):
    return built


def oracle(name):
    return lc.expected(ol, name)


def verdicts(name):
    return [(on, failed, reason) for _, _, _, on, failed, reason in oracle(name)]


def entries(c, k):
    return c["idx"][c["off"][k]:c["off"][k + 1]], c["code"][c["off"][k]:c["off"][k + 1]]


def words_of(c, k):
    w = lc.rank_of(c)[entries(c, k)[0]] // 64
    return int(w.min()), int(w.max())


@pytest.mark.parametrize("name", list(lc.CASES))
def test_restatement_reproduces_the_oracle(name):
    for ci, (o, r, fate, on, failed, reason) in enumerate(oracle(name)):
        assert lc.same_partitions(r, o), (name, ci)
        assert np.array_equal(fate, o["fate"]), (name, ci)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_domain(name):
    """ranks are not read indices, equal starts occur, every column has >= 3 entries"""
    for c in lc.get(name)["contigs"]:
        n = len(c["read_start"])
        assert np.all(np.diff(c["off"]) >= 3)
        if n >= 16:
            assert not np.array_equal(lc.rank_of(c), np.arange(n)) and len(np.unique(c["read_start"])) < n


@pytest.mark.parametrize("name", list(lc.CASES))
def test_harness_host_form_equals_the_oracle(name, tmp_path):
    case = lc.get(name)
    fin, fout = str(tmp_path / "in.i64"), str(tmp_path / "out.i64")
    lc.to_i64(case).tofile(fin)
    subprocess.run([HARNESS, "loop_a", fin, fout], check=True)
    got = lc.from_i64(np.fromfile(fout, np.int64), case)
    for ci, (g, (o, r, _, _, _, _)) in enumerate(zip(got, oracle(name))):
        assert np.array_equal(g["rec"][:, :4], o["rec"]), (name, ci)
        for k in ("state", "more", "less"):
            assert np.array_equal(g[k], o[k]), (name, ci, k)
        assert np.array_equal(g["rec"][:, 4:7], r["rec"][:, 4:7]), (name, ci, "lo / hi / reach")


def test_reads():
    c = lc.get("reads")["contigs"]
    assert [len(x["read_start"]) for x in c] == [2048, 2049, 64, 65]
    assert verdicts("reads") == [(1, 0, None), (0, 0, None), (1, 0, None), (1, 0, None)]
    o = oracle("reads")[0][0]
    last = int(np.argmax(lc.rank_of(c[0])))                               # the read of rank 2047: word 31, bit 63
    assert o["state"][1, last] != 2 and o["fate"][3].tolist() == [1, 1]    # in a partition that was augmented
    assert words_of(c[3], 2) == (0, 1) and words_of(c[2], 2) == (0, 0)     # N = 65: the column lies over words 0 | 1


def test_words():
    cs = lc.get("words")["contigs"]
    assert verdicts("words") == [(1, 0, None), (1, 1, "column"), (1, 0, None)]
    for ci, c in enumerate(cs):
        fate = oracle("words")[ci][0]["fate"]
        spans = [words_of(c, k) for k in range(len(c["pos"]))]
        for ww in (1, 2, 3, 4):      # created and augmented at every width, with entries on both sides of each word boundary
            ks = [k for k, (a, b) in enumerate(spans) if b - a + 1 == ww]
            assert {int(fate[k, 0]) for k in ks} >= {1, 2}, (ci, ww)
            rk = lc.rank_of(c)[entries(c, ks[0])[0]]
            for b in range(spans[ks[0]][0] + 1, spans[ks[0]][1] + 1):
                assert 64 * b - 1 in rk and 64 * b in rk
        five = [k for k, (a, b) in enumerate(spans) if b - a + 1 == 5]
        assert len(five) == (0 if ci == 0 else 1)
        if ci == 1:
            assert fate[five[0], 0] == 2                                   # looked at: the kernel must hand the contig back
        if ci == 2:
            assert fate[five[0], 0] == 0 and fate[five[0] - 1, 0] == 1 and c["pos"][five[0]] - c["pos"][five[0] - 1] <= 5      # skipped by `<= 5`


def test_depth():
    cs = lc.get("depth")["contigs"]
    assert verdicts("depth") == [(1, 0, None), (1, 1, "column")]
    for ci, c in enumerate(cs):
        n = np.diff(c["off"]); fate = oracle("depth")[ci][0]["fate"]
        for d in (64, 65, 128) + ((129,) if ci else ()):
            assert {int(fate[k, 0]) for k in np.flatnonzero(n == d)} == {1, 2}, (ci, d)
        assert n.max() == (129 if ci else 128)


def test_codes():
    case = lc.get("codes")
    cs, kinds = case["contigs"], case["kinds"]
    v = verdicts("codes")
    assert v[0] == (1, 0, None) and v[1] == (1, 1, "column") and all(x == (1, 0, None) for x in v[2:])
    assert len(np.unique(entries(cs[0], 0)[1])) == 15 and len(np.unique(entries(cs[1], 0)[1])) == 16
    k = kinds.index("ref_absent")
    assert cs[k]["k0"][0] not in entries(cs[k], 0)[1] and oracle("codes")[k][0]["fate"][1].tolist() == [1, 0]
    o = oracle("codes")[k][0]
    assert set(np.unique(o["state"][0]).tolist()) == {-1, 0, 2}           # no read carries the reference code: nobody is +1
    k = kinds.index("ref_high")
    cmp_ = oracle("codes")[k][0]["cmp"]
    assert cs[k]["k0"][0] >= 128 and np.any(cmp_["second"] == cs[k]["k0"][0])      # the reference code taken for the second allele (:838)
    # the tie windows: order bytes as the table says, and per window a wrong tie rule that yields other partitions
    for kind in ("tie_fast", "tie_amb", "tie_keys7"):
        other = {"lowest": 0, "first": 0}
        for ci in [i for i, x in enumerate(kinds) if x == kind]:
            c = cs[ci]; o, r = oracle("codes")[ci][:2]
            assert r["n_ties"] >= 1
            code = entries(c, 2)[1]
            tied = [int(x) for x in np.unique(code) if (code == x).sum() in (4, 5) and x != lc.A_]
            assert len(tied) == 2
            same_byte = lc.order_byte(tied[0]) == lc.order_byte(tied[1])
            assert same_byte == (kind == "tie_amb")
            assert (len(np.unique(code)) >= 7) == (kind == "tie_keys7")
            for rule in other:
                w = lc.restate(c, lc.tap_seconds(o), tie=rule)[0]
                other[rule] += 0 if lc.same_partitions(w, o) else 1
        # (keys of equal order byte share a bucket and iterate in the order they were inserted: there "first appearance" IS the reference's rule)
        assert other["lowest"] > 0 and (other["first"] > 0) == (kind != "tie_amb"), (kind, other)


def live_at(o, c, k):
    """partitions created before column k that it can still meet: within 50 kb of their right end and pos < reach (the device's live slots),
    with right / reach as the columns before k left them"""
    right, reach = {}, {}
    for j in range(k):
        f, p = o["fate"][j]
        if f == 0:
            continue
        e = int(c["read_end"][entries(c, j)[0]].max())
        right[p] = max(right.get(p, -1), int(c["pos"][j])); reach[p] = max(reach.get(p, -1), e)
    pos = int(c["pos"][k])
    return [p for p in right if abs(pos - right[p]) <= 50000 and pos < reach[p]]


def test_slots():
    cs = lc.get("slots")["contigs"]
    assert verdicts("slots") == [(1, 0, None), (1, 1, "slots"), (1, 0, None), (1, 0, None)]
    for ci, c in enumerate(cs):
        o = oracle("slots")[ci][0]
        S = len(c["pos"])
        assert lc.pool_cap(S, lc.DIV) >= 65                               # the pool is not what hands it back
        created = np.flatnonzero(o["fate"][:, 0] == 2)
        assert len(created) == (64 if ci == 0 else 65)
        k = int(created[-1])
        # live partitions when the last one is created: 63 (ci 0: it is the 64th), 64 (no room for a 65th), 63 after one died
        assert len(live_at(o, c, k)) == (63, 64, 63, 63)[ci]
        if ci >= 2:      # it died exactly here: it was live at the column before
            assert len(live_at(o, c, k - 1)) == 64
            dead = (set(live_at(o, c, k - 1)) - set(live_at(o, c, k))).pop()
            if ci == 2:
                assert int(c["pos"][k]) == int(c["read_end"][o["state"][dead] != 2].max())             # pos = reach
            else:
                assert int(c["pos"][k]) - int(o["rec"][dead, 1]) == 50001 and np.any((o["cmp"]["col"] == k) & (o["cmp"]["kind"] == 0))


def test_pool():
    case = lc.get("pool")
    assert case["cap"] == lc.pool_cap(case["k"], case["pool_div"]) == 49
    assert [len(c["pos"]) for c in case["contigs"]] == [case["k"]] * 2
    assert [len(x[0]["rec"]) for x in oracle("pool")] == [case["cap"], case["cap"] + 1]
    assert verdicts("pool") == [(1, 0, None), (1, 1, "pool")]
    for ci, c in enumerate(case["contigs"]):      # never more than a few live partitions: the slots are not what hands it back
        o = oracle("pool")[ci][0]
        assert max(len(live_at(o, c, int(k))) for k in np.flatnonzero(o["fate"][:, 0] == 2)) < 8


def test_ring():
    cs = lc.get("ring")["contigs"]
    assert verdicts("ring") == [(1, 0, None), (1, 1, "ring"), (1, 0, None)]
    for ci, c in enumerate(cs):
        spans = [words_of(c, k) for k in range(len(c["pos"]))]
        assert all(b - a + 1 <= 4 for a, b in spans)
        hi = 0; worst = 0
        for a, b in spans:
            hi = max(hi, b + 1); worst = max(worst, hi - a)
        assert worst == (8, 9, 4)[ci]
    c = cs[2]; o = oracle("ring")[2][0]
    assert len(o["rec"]) == 1 and np.all(o["fate"][1:, 0] == 1)
    rk = lc.rank_of(c)
    fresh = np.flatnonzero((rk >= 576) & (rk < 579))                      # joined in word 9, lanes 0..2
    stale = np.flatnonzero((rk >= 64) & (rk < 67))                        # word 1, the same lanes: more - less > 0 when the others join
    assert np.all(o["more"][0, fresh] == 2) and np.all(o["less"][0, fresh] == 0) and np.all(o["more"][0, stale] - o["less"][0, stale] >= 2)


def test_counters():
    cs = lc.get("counters")["contigs"]
    assert verdicts("counters") == [(1, 0, None), (1, 1, "counter"), (1, 0, None)]
    for ci, want in ((0, 255), (1, 256)):
        o = oracle("counters")[ci][0]
        assert len(o["rec"]) == 1 and o["more"][0].max() == want and o["less"][0].max() == 0 and np.all(np.diff(cs[ci]["pos"]) == 6)
    c = cs[2]; o = oracle("counters")[2][0]
    r12 = int(np.flatnonzero(lc.rank_of(c) == 12)[0])
    # the read of rank 12 column by column, through the restatement stopped after each column
    seen = []
    for k in range(2, 6):
        sub = {**c, "pos": c["pos"][:k], "k0": c["k0"][:k], "off": c["off"][:k + 1]}
        r = lc.restate(sub, lc.tap_seconds(o))[0]
        seen.append((int(r["state"][0, r12]), int(r["more"][0, r12]), int(r["less"][0, r12])))
    assert seen == [(0, 0, 0), (-1, 1, 0), (-1, 1, 1), (1, 2, 1)]          # fresh without a vote; votes; opposed at 1; opposed at 0: turns over
    assert np.all(o["fate"][1:7, 0] == 1) and np.all(o["fate"][1:7, 1] == 0)
    t = {int(col): (int(a), int(b), int(d), int(e)) for col, a, b, d, e in zip(o["cmp"]["col"], o["cmp"]["n00"], o["cmp"]["n01"], o["cmp"]["n10"], o["cmp"]["n11"]) if col in (5, 6)}
    assert t[5][1] > 0 and t[5][2] > 0 and t[5][0] == 0 and t[5][3] == 0   # reference code C against the partition's phase: swapped < 0
    code6 = entries(c, 6)[1]
    assert (code6 == lc.A_).sum() == (code6 == lc.C_).sum()                # nA == na


def test_rules():
    case = lc.get("rules")
    cs, kinds = case["contigs"], case["kinds"]
    res = oracle("rules")
    assert all(v == (1, 0, None) for v in verdicts("rules"))
    fate = lambda kind: res[kinds.index(kind)][0]["fate"][:, 0].tolist()
    assert fate("gap5") == [2, 1, 0, 2, 1] and fate("gap6") == [2, 1, 2, 1, 1]
    g6 = kinds.index("gap6")
    assert cs[g6]["pos"][3] - cs[g6]["pos"][2] == 3                        # 3 behind a column that only created a partition: still looked at
    wrong = lc.restate(cs[g6], {}, last_on_create=True)[0]
    assert not lc.same_partitions(wrong, res[g6][0])                       # last_position moved on create as well: other partitions
    assert fate("far50000") == [2, 1, 1] and fate("far50001") == [2, 1, 2]
    assert res[kinds.index("far50001")][0]["cmp"]["kind"].tolist().count(0) == 1
    for d, kind in ((-1, "reach-1"), (0, "reach0")):
        k = kinds.index(kind); c = cs[k]; o = res[k][0]
        reach = int(c["read_end"][o["state"][0] != 2].max())
        assert int(c["pos"][2]) == reach + d
        shared = int((o["state"][0, entries(c, 2)[0]] != 2).sum())
        assert shared == (1 if d == -1 else 0)
    assert fate("half13") == [2, 1, 1] and fate("half15") == [2, 1, 2]
    for kind, n in (("half13", 13), ("half15", 15)):
        k = kinds.index(kind)
        assert len(entries(cs[k], 2)[0]) == n
        cm = res[k][0]["cmp"]
        sel = cm["col"] == 2
        assert int((cm["n00"] + cm["n01"] + cm["n10"] + cm["n11"])[sel][0]) == 6
    # the prescribed tables are what the (partition, column) pair yields, and they sit where the table of cases says
    tabs = case["tables"]
    first = kinds.index("table")
    cats = {}
    sides = {c: set() for c in (10, 30, 70, 110)}
    for t, (o, _, _, _, _, _) in zip(tabs, res[first:]):
        cm = o["cmp"]
        k = int(np.flatnonzero(cm["col"] == 2)[0])
        got = (int(cm["n00"][k]), int(cm["n01"][k]), int(cm["n10"][k]), int(cm["n11"][k]))
        assert got == tuple(t), (t, got)
        est = lc.float_estimate(t)
        if est is not None:
            key = ("in" if 13 <= est <= 17 else "out", bool(cm["chi"][k] > 15))
            cats[key] = cats.get(key, 0) + 1
        n00, n01, n10, n11 = t
        c = sum(t)
        if c in sides:
            for x in (n00 + n01, n01 + n11):
                sides[c] |= {("gt01", x > 0.1 * c), ("lt09", x < 0.9 * c)}
        if n00 + n01 in sides:
            sides[n00 + n01].add(("le01", n01 <= max(0.1 * (n00 + n01), 1.0)))
    # (the double products 0.1 c and 0.9 c of these totals are the exact tenths: the tables decide by the comparison's direction alone)
    assert all(0.1 * c == c // 10 and 0.9 * c == 9 * c // 10 for c in sides)
    assert all(cats.get(k, 0) >= 10 for k in (("in", True), ("in", False), ("out", True), ("out", False))), cats
    for c, s in sides.items():
        assert s >= {("gt01", True), ("gt01", False), ("lt09", True), ("lt09", False), ("le01", True), ("le01", False)}, (c, s)




@pytest.mark.parametrize("name,n", [("many65", 65), ("many129", 129)])
def test_many(name, n):
    case = lc.get(name)
    assert len(case["contigs"]) == n and case["bound"] == 12
    v = verdicts(name)
    S = [len(c["pos"]) for c in case["contigs"]]
    assert sum(1 for s in S if s == 0) >= 5 and sum(1 for s in S if s > 12) >= 3
    assert all(on == (1 if 0 < s <= 12 else 0) for (on, _, _), s in zip(v, S))
    failed = [i for i, (_, f, _) in enumerate(v) if f]
    assert len(failed) >= 3 and all(v[i][2] == "column" for i in failed)
    assert any(v[i - 1] == (1, 0, None) and v[i + 1][0:2] in ((1, 0), (0, 0)) for i in failed)      # handed-back contigs in between
    assert failed[-1] >= 64 if n > 65 else True                            # one behind the first round of 64 lanes of the scans
