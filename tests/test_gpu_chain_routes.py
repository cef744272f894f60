"""The clustering chain of stage 4 -- k_cw_seed_sets, k_cw_seeded_lanes / _rows / _wave, k_window_tail -- at every route cw_chain picks and either side of
every table limit of the tail, on the inputs of tests/chain_cases.py through hs_sr_run_taps (api.separate_reads_chain_taps). One test per case; a case is
one call. tests/test_cpu_chain_cases.py shows without a GPU that every case is what it claims and derives the counters expected here.

Compared with the oracle's separate_reads_on_contig, all by integer equality: every window's reads, the labels of every per-SNP run, the third run as a
partition, the finished labels of every window (chain_check.compare_chain_with_oracle); and the route counters of the call and n_windows_finished_on_host
with what the case's read counts, run counts and table sizes say they must be."""
import pytest

import chain_cases as cc
import chain_check
import oracle_lib as ol
from test_cpu_chain_cases import analyse

pytestmark = pytest.mark.gpu


def _check(name):
    from hairsplitter_amd import api
    assert tuple(api.SR_ROUTE_COUNTERS) == tuple(cc.ROUTE_KEYS)
    case = cc.get(name)
    facts, routes, on_host = analyse(name)
    out = api.separate_reads_chain_taps(case["contigs"], case["window"], case["error_rate"])
    n_win, n_runs = chain_check.compare_chain_with_oracle(out, case["contigs"], cc.oracle_taps(ol, name))
    assert n_win == len(facts) and n_runs == sum(f["runs"] for f in facts)
    got = {k: out["taps"][k] for k in cc.ROUTE_KEYS}
    assert got == routes, name
    assert out["n_windows_finished_on_host"] == on_host, name
    return out


def test_narrow(built):
    """m = 1, 4, 5, 56 .. 64, 8 / 9 / 12 haplotypes, a window without neighbours, three noisy windows whose labels hang on the lowest-of-equals rule: the
    all_lanes branch; two windows over FIN_GCAP finished on the host"""
    _check("narrow")


def test_mixed(built):
    """m = 64, 65, 255, 256, 300: one run per lane, row units of 8 and 8 + 1, one wavefront per run; 1 .. 62 runs per window; windows whose
    third run hangs on one run of the merged-ids key (the 17th, the 21st, the 56th, the 58th) and on the rounding of the reference's double sum"""
    _check("mixed")


def test_tables(built):
    """kc = 16 | 17, g = 8 | 9, n_links = 16 | 18; links applied and links refused on the device"""
    _check("tables")


def test_alleles(built):
    """seeding columns of 16 and 17 codes: the overflow list at m <= 64, the columns themselves at m = 130 and 256"""
    _check("alleles")


def test_columns(built):
    """column depths 64 | 65, 7 .. 17 columns, id ranges 1024 | 1025, SNP pairs 10 | 11 apart; for each of the column forks a window whose link is
    applied or refused by that column, entry or pair alone"""
    _check("columns")


def test_scratch(built):
    """m = 2048 and 2049 in one call (the tail in LDS and in global scratch), then m = 2048 alone"""
    _check("scratch")
    _check("scratch_alone")
