"""Loop A of stage 3 on the device -- k_loop_a_prepare, k_loop_a, k_loop_a_scan, k_loop_a_pack, queued by the plan / launch / collect code stage 3
uses -- either side of every limit in the header comment of hs_kernels_loopa.hip, on the columns of tests/loop_a_cases.py through hs_loop_a_test
(api.loop_a_test). One test per case; a case is one call per layout of the candidates. tests/test_cpu_loop_a_cases.py shows without a GPU that
every case is what it claims, that the numpy restatement the verdicts come from reproduces the oracle, and that the host form equals the oracle.

All by integer equality: form=device against the oracle's loop A on left, right, numberOfOccurences, number_of_correlating_snps and per read state,
more, less of every partition in creation order; lo / hi / reach against form=host; on_device and failed against what the documented limits, restated
once (loop_a_cases.restate), say for the oracle's own walk -- so a kernel that hands back a contig it should hold fails by `failed` alone; one launch of
k_loop_a in kernel_stats(); the contigs handed back (or never planned) against the oracle through form=host. The candidate bound and the pool divisor
are arguments of the entry: nothing here steers by the environment."""
import numpy as np
import pytest

import loop_a_cases as lc
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _same(got, o, what):
    assert np.array_equal(got["rec"][:, :4], o["rec"]), what
    for k in ("state", "more", "less"):
        assert np.array_equal(got[k], o[k]), what + (k,)


def _check(name):
    from hairsplitter_amd import api
    case = lc.get(name)
    exp = lc.expected(ol, name)
    bound, div = case.get("bound", lc.BOUND), case.get("pool_div", lc.DIV)
    want_on = [e[3] for e in exp]; want_failed = [e[4] for e in exp]
    host = api.loop_a_test(case["contigs"], "host", bound, div)
    assert not host["on_device"].any() and not host["failed"].any()
    for light in (False, True):
        api.kernel_stats_every(1)
        api.kernel_stats_reset()
        dev = api.loop_a_test(case["contigs"], "device", bound, div, light=light)
        assert dev["on_device"].tolist() == want_on, (name, light)
        assert dev["failed"].tolist() == want_failed, (name, light, [e[5] for e in exp])
        assert api.kernel_stats().get("k_loop_a", {}).get("launches", 0) == (1 if any(want_on) else 0), (name, light)
        for ci, e in enumerate(exp):
            g = dev["contigs"][ci]
            if want_on[ci] and not want_failed[ci]:
                _same(g, e[0], (name, light, ci))
                assert np.array_equal(g["rec"][:, 4:7], host["contigs"][ci]["rec"][:, 4:7]), (name, light, ci, "lo / hi / reach")
            else:
                assert len(g["rec"]) == 0, (name, light, ci)
    for ci, e in enumerate(exp):      # every contig through the host form: what the driver walks when the device hands one back
        _same(host["contigs"][ci], e[0], (name, "host", ci))
        assert np.array_equal(host["contigs"][ci]["rec"][:, 4:7], e[1]["rec"][:, 4:7]), (name, "host", ci, "lo / hi / reach")


def test_reads(built):
    """N = 2048 with the read of rank 2047 in a partition; 2049 not planned; 64 and 65"""
    _check("reads")


def test_words(built):
    """columns over 1 .. 4 words created and augmented (each step<WW>); a 5-word column handed back; one behind an augmenting column skipped first"""
    _check("words")


def test_depth(built):
    """columns of 64, 65, 128 entries; 129 handed back"""
    _check("depth")


def test_codes(built):
    """15 | 16 codes; no reference code; a reference code >= 128; tied second alleles on the fast path, with equal order bytes, with 7 keys"""
    _check("codes")


def test_slots(built):
    """64 live partitions; no slot for a 65th; the slot of a partition that died by pos >= reach, or 50 001 behind, reused"""
    _check("slots")


def test_pool(built):
    """partitions created = the pool's cap | one more, the divisor passed in"""
    _check("pool")


def test_ring(built):
    """hi_water - wlo = 8 | 9; fresh reads over stale ring bytes"""
    _check("ring")


def test_counters(built):
    """more - less = 255 | 256; the vote sequences of one read"""
    _check("counters")


def test_rules(built):
    """the `<= 5`, 50 000, reach and n / 2 forks; 268 prescribed 2x2 tables around 0.1 c, 0.9 c and chi-square 15"""
    _check("rules")


def test_many(built):
    """65 and 129 contigs in one call, some without candidates, above the bound or handed back"""
    _check("many65")
    _check("many129")
