"""hs_rules.h -- the reference's small rules as the kernels, the host code and the harness all call them -- against their independent
restatements: computeChiSquare against tests/chi_tables.py on the threshold tables the oracle is held to, the central-base predicate
against the numpy form of the GPU tests, the static hash-map rank against the emulator's home bucket and info byte."""
import os
import subprocess

import numpy as np
import pytest

import chi_tables as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# total 0; one margin empty or full; both margins degenerate -> 0, 0, -1 (call_variants.cpp:1135-1163)
DEGENERATE = [((0, 0, 0, 0), 0.0),
              ((3, 4, 0, 0), 0.0), ((0, 0, 3, 4), 0.0), ((3, 0, 4, 0), 0.0), ((0, 3, 0, 4), 0.0), ((200, 55, 0, 0), 0.0),
              ((7, 0, 0, 0), -1.0), ((0, 7, 0, 0), -1.0), ((0, 0, 7, 0), -1.0), ((0, 0, 0, 7), -1.0), ((0, 0, 0, 255), -1.0)]


@pytest.fixture(scope="module")
def rules(built):
    """(threshold tables, their chi-square bits, the degenerate tables' values, predicate matrix [k0 - 33][k1 - 33], rank rows) from ONE run"""
    rng = np.random.default_rng(5)
    tabs = []
    for thr in (15, 20):
        tabs += ct.exact_tables(thr) + ct.near_tables(thr, 300, rng)
    inp = "".join("%d %d %d %d\n" % t for t in tabs + [t for t, _ in DEGENERATE])
    exe = os.path.join(os.path.dirname(built["harness"]), "rules_selftest")
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    chi = np.array([int(l.split()[1], 16) for l in out if l.startswith("chi ")], np.uint32)
    cbt = np.array([[c == "1" for c in l.split()[1]] for l in out if l.startswith("cbt ")])
    rank = np.array([[int(x) for x in l.split()[1:]] for l in out if l.startswith("rank ")], np.int64)
    assert len(chi) == len(tabs) + len(DEGENERATE)
    return tabs, chi[:len(tabs)], chi[len(tabs):].view(np.float32), cbt, rank


def test_chi_square_equals_the_restatement_bit_for_bit(rules):
    tabs, chi, _, _, _ = rules
    assert len(tabs) >= 344 + 496 + 600
    ref = np.array([ct.chi_square_reference(*t) for t in tabs], np.float32)
    assert np.array_equal(ref.view(np.uint32), chi)
    # (the tables are the ones where rounding alone decides: exact-threshold tables land on both sides)
    v = chi.view(np.float32)
    for thr in (15, 20):
        on = ct.exact_chi(tabs) == thr
        assert np.any(on & (v > thr)) and np.any(on & (v < thr)) and np.any(on & (v == thr))


def test_chi_square_of_degenerate_tables(rules):
    _, _, deg, _, _ = rules
    assert deg.tolist() == [want for _, want in DEGENERATE]


def test_central_base_predicate_equals_the_numpy_restatement(rules):
    from test_gpu_kernels import _central_base_test
    _, _, _, cbt, _ = rules
    codes = np.arange(33, 158)
    assert cbt.shape == (125, 125)
    k0, k1 = np.meshgrid(codes, codes, indexing="ij")
    assert np.array_equal(cbt, _central_base_test(k0, k1))
    assert cbt.any() and not cbt.all()


def test_static_rank_equals_the_emulator(rules):
    """every key alone in a fresh map of 8 and of 16 buckets: rank = home bucket << 5 | 31 - low five bits of the info byte"""
    _, _, _, _, rank = rules
    assert rank.shape == (512, 5)
    key, wide, got, bucket, info = rank.T
    assert np.array_equal(key, np.tile(np.arange(256), 2)) and np.array_equal(wide, np.repeat([0, 1], 256))
    assert np.all((bucket >= 0) & (bucket < np.where(wide == 1, 16, 8)))
    assert np.array_equal(got, (bucket << 5) | (31 - (info & 31)))


# ---- hs_job_rules.h (the rules over a whole job) against hairsplitter_amd/dist.py, through tests/harness/job_rules_selftest.cpp ----
def _near_a_tenth():
    return (0.1 + 0.01 * np.random.default_rng(11).standard_normal(3000)).astype(np.float32)


ERROR_RATE_CASES = [
    ("no entry", np.zeros(0, np.float32)),
    ("no positive entry", np.array([0.0, -1.0, 0.0, -0.25], np.float32)),
    ("one entry", np.array([0.0625], np.float32)),
    ("zeros and negatives interleaved", np.array([0.0, 0.05, -0.3, 0.2, 0.0, 0.1, -1.0, 0.0, 0.07], np.float32)),
    ("float32 running sum differs from the float64 sum", _near_a_tenth()),
    ("above the cap", np.array([0.2], np.float32)),
    ("exactly the cap", np.array([0.15], np.float32)),
    ("%g drops digits", np.array([0.123456789], np.float32)),
]

# (sum of the read lengths, reads, window size with fewer than 20 reads above 4 kb, with 20): separate_reads.cpp:1466-1498
WINDOW_CASES = [
    (0, 0, 2000, 2000),
    (2000 * 200, 200, 2000, 2000),           # mean exactly 2000: neither below nor above it
    (4000 * 200, 200, 2000, 2000),           # mean exactly 4000
    (399900, 200, 500, 2000),                # 1999.5
    (400100, 200, 1000, 2000),               # 2000.5
    (799900, 200, 1000, 2000),               # 3999.5
    ((1 << 31) - 1, 1000000, 1000, 2000),    # the largest sum an int holds: mean 2147.48
    (1 << 31, 1000000, 500, 2000),           # wraps to the most negative int: a negative mean
    ((1 << 32) + 5, 1000000, 500, 2000),     # wraps to 5
]


@pytest.fixture(scope="module")
def job_rules(built):
    """(error-rate lines, window-size lines) of ONE run of the harness program on every case"""
    inp = "".join("er %d %s\n" % (v.size, " ".join("%08x" % b for b in v.view(np.uint32))) for _, v in ERROR_RATE_CASES)
    inp += "".join("ws %d %d %d\n" % (total, n, above) for total, n, _, _ in WINDOW_CASES for above in (19, 20))
    exe = os.path.join(os.path.dirname(built["harness"]), "job_rules_selftest")
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    er = [l.split()[1:] for l in out if l.startswith("er ")]
    ws = [int(l.split()[1]) for l in out if l.startswith("ws ")]
    assert len(er) == len(ERROR_RATE_CASES) and len(ws) == 2 * len(WINDOW_CASES)
    return er, ws


def _f32(bits_hex):
    return np.array([int(bits_hex, 16)], np.uint32).view(np.float32)[0]


def test_job_error_rate_equals_the_python_form_bit_for_bit(job_rules):
    from hairsplitter_amd import dist
    v = ERROR_RATE_CASES[4][1]
    assert np.float32(np.cumsum(v, dtype=np.float32)[-1]) != np.float32(v.astype(np.float64).sum())      # (the case is what it says)
    for (name, v), (er_bits, n_pos, s4_bits) in zip(ERROR_RATE_CASES, job_rules[0]):
        want = np.float32(dist.mean_of_positive_f32(v))
        want_s4 = np.float32(dist.stage4_error_rate(float(want)))
        got, got_s4 = _f32(er_bits), _f32(s4_bits)
        assert int(n_pos) == int((v > 0).sum()), name
        if not (v > 0).any():
            assert np.isnan(want) and np.isnan(got) and np.isnan(want_s4) and np.isnan(got_s4), name
        else:
            assert got.view(np.uint32) == want.view(np.uint32), name
            assert got_s4.view(np.uint32) == want_s4.view(np.uint32), name
    # what the cap and %g do, stated independently of both sides
    s4 = {name: _f32(s) for (name, _), (_, _, s) in zip(ERROR_RATE_CASES, job_rules[0])}
    assert s4["above the cap"] == np.float32(0.15) and s4["exactly the cap"] == np.float32(0.15)
    assert s4["%g drops digits"] == np.float32(0.123457) and s4["one entry"] == np.float32(0.0625)


def test_window_size_from_counts_equals_the_python_form(job_rules):
    from hairsplitter_amd import dist
    got = iter(job_rules[1])
    for total, n, want19, want20 in WINDOW_CASES:
        for above, want in ((19, want19), (20, want20)):
            assert next(got) == dist.window_size_from_counts(total, n, above) == want, (total, n, above)
