"""hs_edlib_align_bytes: edlibAlign on raw bytes with edlib's additionalEqualities (any alphabet up to 256 symbols; the equality
vectors of the path kernels from a table in LDS or in device scratch), and the stage-5 call sites on it -- against today's
four-code path where both answer, against the reference's bundled edlib live (oracle/_ref/edlib_driver, where build() compiled
it) and recorded (tests/golden/edlib_equalities_vectors.json.gz, stage5_bytes_cases.json; pairs from
tests/edlib_alphabet_pairs.py), and against a plain dynamic program over the equality matrix."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edlib_alphabet_pairs as AP  # noqa: E402
import edlib_mode_pairs as P  # noqa: E402
import golden_util as gu  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "edlib_driver")
SYM = "=IDX"
_cache = {}


def _golden():
    if "gold" not in _cache:
        _cache["gold"] = json.loads(gzip.open(os.path.join(gu.GOLD, "edlib_equalities_vectors.json.gz")).read())
    return _cache["gold"]


def _eq_pairs():
    if "eq" not in _cache:
        _cache["eq"] = AP.eq_pairs()
        assert AP.digest(_cache["eq"][0]) == _golden()["eq"]["digest"], "the seeded pairs are not the ones the stored results were made from"
    return _cache["eq"]


def _cigar(ops):
    if ops is None or len(ops) == 0:
        return "*"
    cut = np.flatnonzero(np.diff(ops)) + 1
    runs = np.diff(np.concatenate(([0], cut, [len(ops)])))
    heads = ops[np.concatenate(([0], cut))]
    return "".join("%d%s" % (c, SYM[o]) for c, o in zip(runs.tolist(), heads.tolist()))


def _key(g):
    return (g["distance"], g["n_locations"], g["start"], g["end"], None if g["ops"] is None else g["ops"].tobytes())


def _by_k(api, pairs, ks, **kw):
    """edlib_align of every pair i with bound ks[i] (None: skipped), one call per distinct bound"""
    out = [None] * len(pairs)
    for k in sorted(set(k for k in ks if k is not None)):
        idx = [i for i, x in enumerate(ks) if x == k]
        for i, g in zip(idx, api.edlib_align([pairs[i] for i in idx], k=k, **kw)):
            out[i] = g
    return out


def _by_kind(api, pairs, kinds, ks=None, **kw):
    """the pairs of every kind under the equalities of that kind (one relation per call)"""
    out = [None] * len(pairs)
    for kind in sorted(set(kinds)):
        idx = [i for i, x in enumerate(kinds) if x == kind]
        sub = [pairs[i] for i in idx]
        res = api.edlib_align(sub, equalities=AP.EQUALITIES[kind], **kw) if ks is None else _by_k(api, sub, [ks[i] for i in idx], equalities=AP.EQUALITIES[kind], **kw)
        for i, g in zip(idx, res):
            out[i] = g
    return out


def _dp_distance(q, t, equal, mode):
    """edit distance of the three modes by the textbook recurrence over the equality matrix, a row at a time"""
    cost = ~equal[q][:, t]
    ar = np.arange(len(t) + 1)
    row = np.zeros(len(t) + 1, dtype=np.int64) if mode == "HW" else ar.astype(np.int64)
    for i in range(len(q)):
        tmp = np.empty_like(row)
        tmp[0] = i + 1
        tmp[1:] = np.minimum(row[1:] + 1, row[:-1] + cost[i])
        row = np.minimum.accumulate(tmp - ar) + ar      # a run of deletions after the best cell to the left
    return int(row[-1]) if mode == "NW" else int(row.min())


def _replay(q, t, g, equal):
    """the moves rebuild the query and target[start .. end]; op 0 exactly where the relation holds; the others are the distance"""
    qi, ti, bad = 0, max(g["start"], 0), 0
    for o in g["ops"].tolist():
        if o in (0, 3):
            assert bool(equal[q[qi], t[ti]]) == (o == 0), (qi, ti, o)
            qi += 1; ti += 1
        elif o == 1:
            qi += 1
        else:
            ti += 1
        bad += o != 0
    assert qi == len(q)
    assert ti == g["end"] + 1
    assert bad == g["distance"]


def test_bytes_give_the_answers_of_the_four_code_path(built):
    """Code pairs written as ACGT bytes and under a random renaming to four other bytes, through alphabet="bytes": distance,
    numLocations, start, end and moves of today's path, every mode, TASK_LOC and TASK_PATH (pairs of 1 base to 24 kb); with
    k = d the same, with k = d - 1 nothing, on every third path pair."""
    from hairsplitter_amd import api
    pairs = P.loc_pairs()[:600] + P.path_pairs()
    forms = [[(AP.ACGT[q], AP.ACGT[t]) for q, t in pairs], AP.renamed(pairs)]
    assert not set(forms[1][0][0].tolist()) <= set(b"ACGT")
    path_sub = list(range(600, len(pairs), 3)) + [len(pairs) - 1]
    for mode in P.MODES:
        for task in ("loc", "path"):
            want = api.edlib_align(pairs, mode=mode, task=task)
            for form in forms:
                got = api.edlib_align(form, mode=mode, task=task, alphabet="bytes")
                for i, (g, w) in enumerate(zip(got, want)):
                    assert _key(g) == _key(w), (mode, task, i, len(pairs[i][0]), len(pairs[i][1]))
        d = [want[i]["distance"] for i in path_sub]
        for ks in (d, [x - 1 if x > 0 else None for x in d]):
            base = _by_k(api, [pairs[i] for i in path_sub], ks, mode=mode, task="path")
            for form in forms:
                got = _by_k(api, [form[i] for i in path_sub], ks, mode=mode, task="path", alphabet="bytes")
                for g, w in zip(got, base):
                    assert (g is None) == (w is None)
                    if g is not None:
                        assert _key(g) == _key(w), (mode, ks is d)
            if ks is not d:
                assert all(g is None or g["distance"] == -1 for g in base)


def test_case_equalities_are_the_upper_cased_pair(built):
    """Pairs over ACGTacgt with a = A, c = C, g = G, t = T: exactly today's result on the upper-cased pair. Without the
    equalities the distance is at least as large, and larger on more than half of the pairs."""
    from hairsplitter_amd import api
    pairs = AP.case_pairs()
    up = [(AP.upper(q).tobytes(), AP.upper(t).tobytes()) for q, t in pairs]
    assert len(set(b for q, t in pairs for b in q.tolist() + t.tolist())) == 8
    n_larger = {}
    for mode in P.MODES:
        want = api.edlib_align(up, mode=mode, task="path")
        got = api.edlib_align(pairs, mode=mode, task="path", equalities=AP.EQUALITIES["case"])
        plain = api.edlib_align(pairs, mode=mode, task="loc", alphabet="bytes")
        for i, (g, w, p) in enumerate(zip(got, want, plain)):
            assert _key(g) == _key(w), (mode, i)
            assert p["distance"] >= g["distance"]
        n_larger[mode] = sum(p["distance"] > g["distance"] for g, p in zip(got, plain))
        assert 2 * n_larger[mode] > len(pairs), n_larger


def test_bytes_without_equalities_match_the_reference_edlib(built):
    """Alphabets of 5, 16 (LDS table), 17, 94 and 256 symbols (scratch table; bytes 0 and 255 present), queries of 1 to 4200
    symbols: distance, numLocations, start, end in NW / SHW / HW and the extended CIGAR of HW against the recorded results of
    the reference's edlib, and against the reference itself where build() compiled its driver (printable alphabets)."""
    from hairsplitter_amd import api
    gold = _golden()["bytes"]
    live = os.path.exists(DRIVER)
    for A in AP.BYTE_ALPHABETS:
        pairs = AP.byte_pairs(A)
        rec = gold[str(A)]
        assert AP.digest(pairs) == rec["digest"]
        seen = set(b for q, t in pairs for b in q.tolist() + t.tolist())
        assert len(seen) == A and (A < 256 or {0, 255} <= seen)
        strs = [(q.tobytes().decode("latin-1"), t.tobytes().decode("latin-1")) for q, t in pairs]
        for mode in P.MODES:
            got = api.edlib_align(pairs, mode=mode, task="loc", alphabet="bytes")
            have = [[g["distance"], g["n_locations"], g["start"], g["end"]] for g in got]
            assert have == [r[mode] for r in rec["results"]], (A, mode)
            if live and A <= 94:
                r = subprocess.run([DRIVER], input="".join("%s -1 %s %s\n" % (mode, q, t) for q, t in strs), capture_output=True, text=True, check=True, timeout=120)
                assert [list(map(int, line.split())) for line in r.stdout.splitlines()] == have, (A, mode)
        got = api.edlib_align(pairs, mode="HW", task="path", alphabet="bytes")
        have = [[g["distance"], g["start"], g["end"], _cigar(g["ops"])] for g in got]
        assert have == [r["HWPATH"] for r in rec["results"]], A
        if live and A <= 94:
            r = subprocess.run([DRIVER], input="".join("HWPATH -1 %s %s\n" % (q, t) for q, t in strs), capture_output=True, text=True, check=True, timeout=120)
            lines = [line.split() for line in r.stdout.splitlines()]
            assert [[int(x[0]), int(x[1]), int(x[2]), x[3]] for x in lines] == have, A


def test_non_transitive_equalities_match_the_reference_edlib(built):
    """ACGT + N with N = A, C, G, T and IUPAC codes with the bases they stand for (neither relation is transitive): the recorded
    results of the reference's edlib with these additionalEqualities, every mode, TASK_PATH, k in {-1, d, d - 1}; the distance of
    a plain dynamic program on every pair of at most 400 x 400; the moves replayed against the relation."""
    from hairsplitter_amd import api
    pairs, kinds = _eq_pairs()
    rec = _golden()["eq"]["results"]
    equal = {kind: AP.equal_matrix(AP.EQUALITIES[kind]) for kind in set(kinds)}
    assert not equal["N"][ord("A"), ord("C")] and equal["N"][ord("N"), ord("A")] and equal["N"][ord("C"), ord("N")]
    nb = [(len(q) + 63) // 64 for q, _ in pairs]
    assert any(b <= 8 for b in nb) and any(8 < b <= 16 for b in nb) and any(16 < b <= 32 for b in nb) and any(b > 64 for b in nb)
    assert sum(20 * b * len(t) + 8 * len(t) >= 1 << 20 for b, (_, t) in zip(nb, pairs)) >= 2      # edlib cuts these in halves
    small = [i for i, (q, t) in enumerate(pairs) if len(q) <= 400 and len(t) <= 400]
    assert len(small) >= 150
    for mode in P.MODES:
        got = _by_kind(api, pairs, kinds, mode=mode, task="path")
        for i, (g, r) in enumerate(zip(got, rec)):
            assert [g["distance"], g["n_locations"], g["start"], g["end"], _cigar(g["ops"])] == r[mode]["-1"], (mode, i, len(pairs[i][0]), len(pairs[i][1]))
            _replay(pairs[i][0], pairs[i][1], g, equal[kinds[i]])
        n_differ = sum(r["plain"][mode] != r[mode]["-1"][0] for r in rec)
        assert n_differ >= 0.3 * len(pairs), (mode, n_differ)
        for i in small:
            assert _dp_distance(pairs[i][0], pairs[i][1], equal[kinds[i]], mode) == got[i]["distance"], (mode, i)
        d = [g["distance"] for g in got]
        for kind, ks in (("d", d), ("d-1", [x - 1 if x > 0 else None for x in d])):
            for i, (g, r) in enumerate(zip(_by_kind(api, pairs, kinds, ks, mode=mode, task="path"), rec)):
                w = r[mode][kind]
                assert (g is None) == (w is None)
                if g is not None:
                    assert [g["distance"], g["n_locations"], g["start"], g["end"], _cigar(g["ops"])] == w, (mode, kind, i)


def test_lane_groupings_agree_under_equalities(built):
    """one wavefront per pair (HS_MYERS_NO_GROUPS) gives what the 8 / 16 / 32-lane groupings give"""
    from hairsplitter_amd import api
    pairs, kinds = _eq_pairs()
    grouped = _by_kind(api, pairs, kinds, mode="NW", task="path")
    os.environ["HS_MYERS_NO_GROUPS"] = "1"
    try:
        alone = _by_kind(api, pairs, kinds, mode="NW", task="path")
    finally:
        del os.environ["HS_MYERS_NO_GROUPS"]
    assert [_key(a) for a in alone] == [_key(g) for g in grouped]
    assert [_cigar(a["ops"]) for a in alone] == [r["NW"]["-1"][4] for r in _golden()["eq"]["results"]]


def test_scratch_table_under_equalities_and_a_call_wide_alphabet(built):
    """One more pair that holds all 256 byte values puts the whole call on the scratch table (equality rows of eight words);
    the symbols a pair does not hold change nothing, so every other pair keeps the recorded result of the reference's edlib."""
    from hairsplitter_amd import api
    pairs, kinds = _eq_pairs()
    rec = _golden()["eq"]["results"]
    filler = (np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8)[::-1].copy())
    for kind in sorted(set(kinds)):
        idx = [i for i, x in enumerate(kinds) if x == kind]
        for mode in P.MODES:
            got = api.edlib_align([pairs[i] for i in idx] + [filler], mode=mode, task="path", equalities=AP.EQUALITIES[kind])
            assert got[-1]["distance"] > 0
            for i, g in zip(idx, got):
                assert [g["distance"], g["n_locations"], g["start"], g["end"], _cigar(g["ops"])] == rec[i][mode]["-1"], (kind, mode, i)


def test_stage5_call_sites_on_any_alphabet(built):
    """reattach_ends / trim_polished with alphabet="bytes" against the reference's code around its edlib: backbones with N runs,
    soft-masked lower case and IUPAC codes (the pair today's path refuses among them), and every case today's path answers."""
    from hairsplitter_amd import api
    gold = json.load(open(os.path.join(gu.GOLD, "stage5_bytes_cases.json")))
    assert AP.cases_digest(AP.stage5_cases()) == gold["digest"]
    cases = gold["cases"]
    refused = [c for c in json.load(open(os.path.join(gu.GOLD, "stage5_alphabet_cases.json"))) if c["kind"] == "refused"]
    assert refused and all(any(c.get("backbone") == r["backbone"] and c.get("consensus") == r["consensus"] for c in cases) for r in refused)
    for name in (None, "stage5_alphabet_cases.json", "stage5_edlib_cases.json"):
        if name is not None:
            cases = json.load(open(os.path.join(gu.GOLD, name)))
        re_ = [c for c in cases if c["kind"] == "reattach"]
        tr = [c for c in cases if c["kind"] == "trim"]
        assert len(re_) >= 40 and len(tr) >= 40
        assert api.reattach_ends([c["backbone"] for c in re_], [c["consensus"] for c in re_], alphabet="bytes") == [c["expected"] for c in re_]
        assert api.trim_polished([c["to_polish"] for c in tr], [c["newcontig"] for c in tr], [c["overhang_left"] for c in tr], [c["overhang_right"] for c in tr],
                                 alphabet="bytes") == [c["expected"] for c in tr]
        if name is None:
            assert any(len(c["expected"]) < len(c["newcontig"]) for c in tr)
            assert sum(len(set(c["backbone"] + c["consensus"])) > 4 for c in re_) >= 20


def test_bytes_arguments(built):
    """n_equalities < 0 is refused; an empty query or target behaves as in hs_edlib_align (edlib.cpp:161-180); an equality that
    names bytes no sequence holds changes nothing."""
    from hairsplitter_amd import api
    from hairsplitter_amd.api import HsError
    import torch
    lib = api.load()
    z = torch.zeros(16, dtype=torch.int32, device="cuda:0")
    s = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    off = np.array([0, 4], np.int64)
    oo = np.array([0, 8], np.int64)
    eq = np.array([[65, 78]], np.uint8)
    call = lambda eqp, n: lib.hs_edlib_align_bytes(api._p(s), api._hp(off, C.c_int64), api._p(s), api._hp(off, C.c_int64), C.c_int32(1), C.c_int32(0), C.c_int32(1),
                                                    C.c_int32(-1), eqp, C.c_int32(n), api._p(z), api._p(z), api._p(z), api._p(z), C.c_void_p(0),
                                                    api._hp(oo, C.c_int64), C.c_void_p(0), C.c_void_p(0))
    with pytest.raises(HsError):
        api._check(call(api._hp(eq, C.c_uint8), -1))
    with pytest.raises(HsError):
        api._check(call(None, 1))
    api._check(call(api._hp(eq, C.c_uint8), 1))
    cases = [("", ""), ("", "ACGTN"), ("ACN", ""), ("", "A")]
    for mode in P.MODES:
        for k in (-1, 0, 2, 10):
            for task in ("distance", "loc", "path"):
                for eqs in (None, AP.EQUALITIES["N"]):
                    got = api.edlib_align(cases, mode=mode, task=task, k=k, alphabet="bytes", equalities=eqs)
                    for (q, t), g in zip(cases, got):
                        dist = max(len(q), len(t)) if mode == "NW" else len(q)
                        end = len(t) - 1 if mode == "NW" else -1
                        assert (g["distance"], g["n_locations"], g["start"], g["end"]) == (dist, 1, -1, end), (mode, k, task, q, t)
                        if task == "path":
                            assert len(g["ops"]) == 0
    pairs, kinds = _eq_pairs()
    sub = [p for p, kind in zip(pairs, kinds) if kind == "N"][:60]
    for eqs, extra in ((None, [("#", "A"), ("#", "%")]), (AP.EQUALITIES["N"], AP.EQUALITIES["N"] + [("n", "A"), (0, 255)])):
        a = api.edlib_align(sub, mode="HW", task="path", alphabet="bytes", equalities=eqs)
        b = api.edlib_align(sub, mode="HW", task="path", equalities=extra)
        assert [_key(x) for x in a] == [_key(x) for x in b]
