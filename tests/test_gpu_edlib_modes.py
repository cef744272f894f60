"""hs_edlib_align: edlibAlign in all three modes (NW / SHW / HW), with the distance bound k and the three tasks, against the
reference's bundled edlib -- live through oracle/_ref/edlib_driver where build() compiled it, and always against its recorded
results (tests/golden/edlib_modes_loc_vectors.json.gz, edlib_nw_shw_path_vectors.json.gz; pairs from tests/edlib_mode_pairs.py)."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edlib_mode_pairs as P  # noqa: E402
import golden_util as gu  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "edlib_driver")
SYM = "=IDX"


def _loc_golden():
    return json.loads(gzip.open(os.path.join(gu.GOLD, "edlib_modes_loc_vectors.json.gz")).read())


def _path_golden():
    return json.loads(gzip.open(os.path.join(gu.GOLD, "edlib_nw_shw_path_vectors.json.gz")).read())


def _cigar(ops):
    if ops is None or len(ops) == 0:
        return "*"
    cut = np.flatnonzero(np.diff(ops)) + 1
    runs = np.diff(np.concatenate(([0], cut, [len(ops)])))
    heads = ops[np.concatenate(([0], cut))]
    return "".join("%d%s" % (c, SYM[o]) for c, o in zip(runs.tolist(), heads.tolist()))


def _by_k(api, pairs, mode, ks, task="loc"):
    """edlib_align of every pair i with bound ks[i] (None: skipped), one call per distinct bound"""
    out = [None] * len(pairs)
    for k in sorted(set(k for k in ks if k is not None)):
        idx = [i for i, x in enumerate(ks) if x == k]
        for i, g in zip(idx, api.edlib_align([pairs[i] for i in idx], mode=mode, task=task, k=k)):
            out[i] = g
    return out


def _replay(q, t, g):
    """the moves rebuild the query and target[start .. end]; their non-matches are the distance"""
    ops = g["ops"]
    qi, ti = 0, max(g["start"], 0)
    bad = 0
    for o in ops.tolist():
        if o in (0, 3):
            assert (q[qi] == t[ti]) == (o == 0), (qi, ti, o)
            qi += 1; ti += 1
        elif o == 1:
            qi += 1
        else:
            ti += 1
        bad += o != 0
    assert qi == len(q)
    assert ti == g["end"] + 1
    assert bad == g["distance"]


def test_edlib_align_locations_match_the_reference_edlib(built):
    """About 2000 seeded pairs of 1-3000 bases (0-30 % edits, queries longer than targets, identical, unrelated and repeat
    pairs), every mode, k in {-1, 0, d - 1, d, d + 1}: distance, numLocations, start and end locations of TASK_LOC."""
    from hairsplitter_amd import api
    gold = _loc_golden()
    pairs = P.loc_pairs(gold["seed"], gold["n"])
    assert P.digest(pairs) == gold["digest"], "the seeded pairs are not the ones the stored results were made from"
    strs = [(P.to_str(q), P.to_str(t)) for q, t in pairs]
    live = os.path.exists(DRIVER)
    n_checked = 0
    for mode in P.MODES:
        res = gold["results"][mode]
        d = [r[0] for r in res["-1"]]
        for kind in P.K_KINDS:
            ks = [P.k_of(kind, d[i]) for i in range(len(pairs))]
            want = res[kind]
            if live:      # the reference's edlib itself, on the same lines the stored results came from
                idx = [i for i, k in enumerate(ks) if k is not None]
                r = subprocess.run([DRIVER], input="".join("%s %d %s %s\n" % (mode, ks[i], *strs[i]) for i in idx),
                                   capture_output=True, text=True, check=True, timeout=600)
                lines = r.stdout.splitlines()
                assert len(lines) == len(idx)
                for i, line in zip(idx, lines):
                    assert list(map(int, line.split())) == want[i], (mode, kind, i)
            got = _by_k(api, pairs, mode, ks)
            for i, (g, w) in enumerate(zip(got, want)):
                assert (g is None) == (w is None)
                if g is None:
                    continue
                assert [g["distance"], g["n_locations"], g["start"], g["end"]] == w, (mode, kind, i, len(pairs[i][0]), len(pairs[i][1]))
                n_checked += 1
    assert n_checked > 20000
    # TASK_DISTANCE: the same distance and end location, no start location (edlib.cpp:223-224)
    sub = pairs[:300]
    for mode in P.MODES:
        loc = api.edlib_align(sub, mode=mode, task="loc")
        dist = api.edlib_align(sub, mode=mode, task="distance")
        for a, b in zip(loc, dist):
            assert (b["distance"], b["end"], b["n_locations"], b["start"], b["ops"]) == (a["distance"], a["end"], a["n_locations"], -1, None)


def test_edlib_align_empty_sequences_as_edlib(built):
    """edlib.cpp:161-180: an empty query or target gives NW max(|q|, |t|) ending at the last target column, SHW / HW the query
    length ending at -1; one location, no start location, no alignment -- whatever k is."""
    from hairsplitter_amd import api
    cases = [("", ""), ("", "ACGT"), ("ACG", ""), ("", "A")]
    for mode in P.MODES:
        for k in (-1, 0, 2, 10):
            for task in ("distance", "loc", "path"):
                got = api.edlib_align(cases, mode=mode, task=task, k=k)
                for (q, t), g in zip(cases, got):
                    dist = max(len(q), len(t)) if mode == "NW" else len(q)
                    end = len(t) - 1 if mode == "NW" else -1
                    assert (g["distance"], g["n_locations"], g["start"], g["end"]) == (dist, 1, -1, end), (mode, k, task, q, t)
                    if task == "path":
                        assert len(g["ops"]) == 0


def test_edlib_align_paths_match_the_reference_edlib(built):
    """NW and SHW paths (and HW) move by move against the reference's edlib (TASK_PATH), pairs of 1 base to 24 kb -- those of
    20 kb and more go through edlib's Hirschberg cuts -- all in ONE call per mode, so that every lane grouping (8 / 16 / 32
    lanes per pair and a wavefront per pair) runs in it. With k = d the same path; the numpy restatement of obtainAlignment
    (oracle/edlib_path_oracle.py) agrees on target[start .. end]."""
    from hairsplitter_amd import api
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import edlib_path_oracle as eo
    gold = _path_golden()
    vec = gold["vectors"]
    assert P.digest(P.path_pairs()) == gold["digest"]
    pairs = [(v["query"], v["target"]) for v in vec]
    nb = [(len(q) + 63) // 64 for q, _ in pairs]
    assert any(b <= 8 for b in nb) and any(8 < b <= 16 for b in nb) and any(16 < b <= 32 for b in nb) and any(b > 32 for b in nb)
    assert sum(len(q) >= 20000 and len(t) >= 20000 for q, t in pairs) >= 3
    for mode in P.MODES:
        got = api.edlib_align(pairs, mode=mode, task="path", cigar="extended")
        for (q, t), v, g in zip(pairs, vec, got):
            w = v[mode]
            assert (g["distance"], g["n_locations"], g["start"], g["end"]) == (w["distance"], w["n_locations"], w["start"], w["end"]), (mode, len(q), len(t))
            assert _cigar(g["ops"]) == w["cigar"], (mode, len(q), len(t))
            assert g["cigar"] == (w["cigar"] if w["cigar"] != "*" else "")
        if mode != "HW":
            for (q, t), g in zip(pairs, got):
                if len(q) * len(t) <= 1500 * 1500:
                    ops = eo._obtain_alignment(eo._codes(q), eo._codes(t)[g["start"]:g["end"] + 1], g["distance"], {"leaves": 0, "splits": 0})
                    assert g["ops"].tolist() == ops, (mode, len(q), len(t))
        # a bound at the distance changes nothing; one below it leaves no path
        d = [g["distance"] for g in got]
        for g, a in zip(_by_k(api, pairs, mode, d, task="path"), got):
            assert (g["distance"], g["n_locations"], g["start"], g["end"]) == (a["distance"], a["n_locations"], a["start"], a["end"])
            assert np.array_equal(g["ops"], a["ops"])
        for g in _by_k(api, pairs, mode, [x - 1 if x > 0 else None for x in d], task="path"):
            if g is not None:
                assert (g["distance"], g["n_locations"], g["start"], g["end"], len(g["ops"])) == (-1, 0, -1, -1, 0)
    # one wavefront per pair gives the same
    os.environ["HS_MYERS_NO_GROUPS"] = "1"
    try:
        alone = api.edlib_align(pairs, mode="NW", task="path")
    finally:
        del os.environ["HS_MYERS_NO_GROUPS"]
    assert [_cigar(a["ops"]) for a in alone] == [v["NW"]["cigar"] for v in vec]


def test_edlib_align_path_invariants_and_hw_equals_edlib_hw_align(built):
    """For every pair and mode: the moves rebuild the query and target[start .. end], their non-matches are the distance, the
    locations are those of TASK_LOC; HW with k = -1 is hs_edlib_hw_align exactly."""
    from hairsplitter_amd import api
    pairs = P.loc_pairs()[:600] + [(v["query"], v["target"]) for v in _path_golden()["vectors"]]
    as_codes = lambda s: np.frombuffer(s.encode(), np.uint8) if isinstance(s, str) else s
    codes = [(as_codes(q), as_codes(t)) for q, t in pairs]
    for mode in P.MODES:
        got = api.edlib_align(pairs, mode=mode, task="path")
        loc = api.edlib_align(pairs, mode=mode, task="loc")
        for (q, t), g, l in zip(codes, got, loc):
            assert (g["distance"], g["n_locations"], g["start"], g["end"]) == (l["distance"], l["n_locations"], l["start"], l["end"])
            if mode == "NW":
                assert (g["start"], g["end"]) == (0, len(t) - 1)
            elif mode == "SHW":
                assert g["start"] == 0
            _replay(q, t, g)
        if mode == "HW":
            as_str = lambda s: s if isinstance(s, str) else P.to_str(s)
            hw = api.edlib_hw_align([(as_str(q), as_str(t)) for q, t in pairs])
            for g, h in zip(got, hw):
                assert (g["distance"], g["start"], g["end"]) == (h["distance"], h["start"], h["end"])
                assert np.array_equal(g["ops"], h["ops"])


def test_edlib_align_string_alphabets(built):
    """Strings are coded per pair by first appearance (as stage 5 codes them): any four bytes behave as edlib's byte equality;
    a fifth distinct byte is an error, not an approximation."""
    from hairsplitter_amd import api
    from hairsplitter_amd.api import HsError
    a = api.edlib_align([("ACGTTGCA", "TTACGTAGCATT")], mode="HW")[0]
    b = api.edlib_align([("acgNNgca", "NNacgNagcaNN")], mode="HW")[0]
    c = api.edlib_align([(b"ACGTTGCA", b"TTACGTAGCATT")], mode="HW")[0]
    assert (a["distance"], a["start"], a["end"], a["ops"].tolist()) == (b["distance"], b["start"], b["end"], b["ops"].tolist())
    assert (a["distance"], a["start"], a["end"], a["ops"].tolist()) == (c["distance"], c["start"], c["end"], c["ops"].tolist())
    with pytest.raises(HsError):
        api.edlib_align([("ACGTN", "ACGT")])
