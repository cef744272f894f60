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
