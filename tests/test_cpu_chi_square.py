"""The oracle's computeChiSquare at the thresholds of loops C and D: on every 2x2 table whose chi-square is exactly 15 or 20 (total <= 255)
and on tables near them, its value is the numpy restatement's, bit for bit (the GPU tests of K4 trust the oracle there)."""
import numpy as np

import chi_tables as ct
import oracle_lib as ol


def test_exact_threshold_tables_are_enumerated():
    """the enumeration in exact integer arithmetic: up to a total of 160 reads 344 tables at 15 and 496 at 20, each exact"""
    for thr, n160 in ((15, 344), (20, 496)):
        tabs = ct.exact_tables(thr)
        assert sum(1 for t in tabs if sum(t) <= 160) == n160
        assert np.all(ct.exact_chi(tabs) == thr)


def test_oracle_chi_square_equals_the_restatement(built):
    case, nr, tabs, routes = ct.table_case()
    keep, chi, tab = ol.column_partition_test(n_reads_of_contig=nr, **case)
    lo = case["col_k0"] < 128
    assert np.array_equal(tab[lo], tabs[lo])
    ref = np.array([ct.chi_square_reference(*(int(x) for x in t)) for t in tab], np.float32)
    assert np.array_equal(ref.view(np.uint32), chi.view(np.uint32))
    # the rounding alone decides: exact-threshold tables that land on both sides of the threshold
    for thr in (15, 20):
        on = lo & (ct.exact_chi(tab) == thr)
        assert np.any(on & (chi > thr)) and np.any(on & (chi < thr)) and np.any(on & (chi == thr))
