"""hs_alignment_to_cigar (host code) against a numpy restatement of edlibAlignmentToCigar (the reference's edlib.cpp:299-349),
and the per-pair coding of strings that api.edlib_align hands to the device."""
import numpy as np
import pytest


def _restated(ops, fmt):
    """edlibAlignmentToCigar: moves 0 '=', 1 'I', 2 'D', 3 'X'; STANDARD writes '=' and 'X' as 'M'; runs of the same character
    as <count><character>; an empty alignment gives an empty string"""
    sym = np.frombuffer(b"MIDM" if fmt == "standard" else b"=IDX", dtype=np.uint8)[np.asarray(ops, np.uint8)]
    if len(sym) == 0:
        return ""
    cut = np.flatnonzero(sym[1:] != sym[:-1]) + 1
    starts = np.concatenate(([0], cut))
    runs = np.diff(np.concatenate((starts, [len(sym)])))
    return "".join("%d%s" % (n, chr(c)) for n, c in zip(runs.tolist(), sym[starts].tolist()))


def test_alignment_to_cigar_matches_edlib_restatement(built):
    from hairsplitter_amd import api
    cases = [[], [0], [1], [2], [3], [0, 3], [3, 0, 0, 3], [1, 1, 2, 2, 1], [0] * 12, [3] * 100 + [0] * 1000 + [2]]
    rng = np.random.default_rng(7)
    for n in (2, 5, 17, 64, 300, 5000):
        cases.append(rng.integers(0, 4, size=n).tolist())
        cases.append(np.repeat(rng.integers(0, 4, size=n), rng.integers(1, 30, size=n)).tolist())
    for ops in cases:
        for fmt in ("standard", "extended"):
            assert api.alignment_to_cigar(np.asarray(ops, np.uint8), fmt) == _restated(ops, fmt), (ops[:20], fmt)
    assert api.alignment_to_cigar([0, 3, 3, 0, 1, 2, 2], "standard") == "4M1I2D"
    assert api.alignment_to_cigar([0, 3, 3, 0, 1, 2, 2], "extended") == "1=2X1=1I2D"


def test_alignment_to_cigar_rejects_bad_moves(built):
    from hairsplitter_amd import api
    with pytest.raises(api.HsError):
        api.alignment_to_cigar(np.array([0, 4], np.uint8))


def test_edlib_pair_coding():
    from hairsplitter_amd import api
    qs, ts = api._edlib_codes([("ACGT", "TTGA"), ("NNac", "caNN"), (b"xy", b"yx"), (np.array([3, 2], np.uint8), np.array([0, 1], np.uint8)), ("", "")])
    assert [q.tolist() for q in qs] == [[0, 1, 2, 3], [0, 0, 1, 2], [0, 1], [3, 2], []]
    assert [t.tolist() for t in ts] == [[3, 3, 2, 0], [2, 1, 0, 0], [1, 0], [0, 1], []]
    with pytest.raises(api.HsError):
        api._edlib_codes([("ACGT", "N")])
    with pytest.raises(api.HsError):
        api._edlib_codes([(np.array([4], np.uint8), np.array([0], np.uint8))])
