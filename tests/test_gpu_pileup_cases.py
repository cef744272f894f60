"""K0 (k_cigar_scan) and K1 (k_pileup_runs + k_pileup_flagged_records) on the records of tests/pileup_cases.py, in the two layouts the library runs them in:
packed (api.pileup: a record's bytes directly behind the previous one's) and resident (api.CvBatch: every record at an address = contig position mod 128,
K1 per contig range on the batch's prebuilt task slice, through hs_cv_pileup_tap). One test per case. tests/test_cpu_pileup_cases.py shows without a GPU
which forks of the decomposition each case reaches and that the oracle tells a kernel with a defect at such a fork from a right one.

All by integer equality with the oracle's generate_msa: every pileup byte, (q_end, n_err, n_len) per record, the event count; K0's chunk table against
pileup_cases.analyse; and, in the resident layout, that every byte of the pile allocation outside the records -- and every byte, counter and chunk entry
of a record outside the launched contig range -- still holds the pattern it was filled with."""
import numpy as np
import pytest

from test_cpu_pileup_cases import load

pytestmark = pytest.mark.gpu


def _packed(name, ev_sizes=(4096,)):
    from hairsplitter_amd import api
    flat, an, o_pile, o_stats = load(name)
    t = api.device_tensors(flat)
    for ev in ev_sizes:
        pile, stats = api.pileup(t, flat, ev_per_task=ev)
        stats = stats.cpu().numpy()
        assert np.array_equal(pile.cpu().numpy(), o_pile), (name, ev)
        assert np.array_equal(stats[:, :3], o_stats[:, :3]), (name, ev)
        assert np.array_equal(stats[:, 3], an.n_events), (name, ev)


def _resident(name, c0, c1, fill):
    """the contigs [c0, c1) of the case in one call on a fresh batch"""
    from hairsplitter_amd import api
    flat, an, o_pile, o_stats = load(name)
    batch = api.CvBatch(flat)
    try:
        tap = api.cv_pileup_tap(batch, c0, c1, fill)
    finally:
        batch.close()
    n = flat.n_rec
    lead, addr, pile = tap["lead"], tap["pile_addr"], tap["pile"]
    span = np.diff(flat.pile_off)
    # the layout: every record at its contig position mod 128, ascending, no overlap, inside the allocation
    assert lead == 256 and len(addr) == n + 1 and len(pile) == lead + int(addr[n]) + 256
    want_mod = (flat.contig_off[flat.rec_contig] + flat.rec_pos) & 127
    assert np.array_equal(addr[:n] & 127, want_mod)
    assert np.all(addr[:n] + span <= addr[1:]) and (n == 0 or addr[0] >= 0)
    assert np.array_equal(tap["rec_chunk_off"], an.chunk_off)
    r0, r1 = int(flat.contig_rec_off[c0]), int(flat.contig_rec_off[c1])
    untouched = np.ones(len(pile), bool)
    for r in range(r0, r1):
        a, b = lead + int(addr[r]), lead + int(addr[r]) + int(span[r])
        assert np.array_equal(pile[a:b], o_pile[int(flat.pile_off[r]):int(flat.pile_off[r + 1])]), (name, r)
        untouched[a:b] = False
    # nothing written outside the records of the range: the bytes in front, the gaps, the records of other contigs, the bytes behind
    spilled = np.flatnonzero(untouched & (pile != fill))
    assert len(spilled) == 0, (name, c0, c1, spilled[:8] - lead, pile[spilled[:8]])
    stats, table = tap["rec_stats"], tap["chunk_table"]
    assert np.array_equal(stats[r0:r1, :3], o_stats[r0:r1, :3])
    assert np.array_equal(stats[r0:r1, 3], an.n_events[r0:r1])
    k0, k1 = int(an.chunk_off[r0]), int(an.chunk_off[r1])
    assert table.shape == an.chunk_table.shape
    assert np.array_equal(table[k0:k1], an.chunk_table[k0:k1])
    first = an.chunk_off[r0:r1][np.diff(an.chunk_off[r0:r1 + 1]) > 0]
    assert int((table[first, 3] & 1).sum()) == int(an.flagged[r0:r1].sum())
    assert np.all(np.delete(stats, np.s_[r0:r1], axis=0) == -1) and np.all(np.delete(table, np.s_[k0:k1], axis=0) == -1)


def _ranges(name):
    """the whole batch in one call; then every contig alone and the two halves of a split in the middle, each on a fresh batch, each with another fill byte"""
    C = load(name)[0].n_contigs
    _resident(name, 0, C, 0xFF)
    if C > 1:
        for k, (c0, c1) in enumerate([(c, c + 1) for c in range(C)] + [(0, C // 2), (C // 2, C)]):
            _resident(name, c0, c1, (0x00, 0x5A, 0xFF)[k % 3])
    else:
        _resident(name, 0, 1, 0x00)


def test_context(built):
    """the 14 contexts of an op's first column inside one chunk, with and without N / P / 0M / 0D / 0I in between"""
    _packed("context")
    _ranges("context")


def test_boundaries(built):
    """the same contexts with the op at index 64, 128 and 256: K0's table carries them over the edge"""
    _packed("boundaries")
    _ranges("boundaries")


def test_pieces(built):
    """tails and contig cuts of every length for M-like and D pieces, later pieces of a deletion, tiny reverse reads, tolerated overhangs: a partial
    piece writes its n bytes and no more"""
    _packed("pieces")
    _ranges("pieces")


def test_windows(built):
    """tasks either side of one and two windows of 256 pieces, ops of more than 512 pieces, a task without a piece, a task beyond the contig end"""
    _packed("windows")
    _ranges("windows")


def test_flags(built):
    """records with a clip between events take the per-event form (at three task sizes), everything else the run form"""
    _packed("flags", (4096, 64, 1 << 30))
    _ranges("flags")


def test_ends(built):
    """records at L - 1, L, L + 5, without ops, of clips only; contigs of 1, 2, 3, 17 bases; a contig without records"""
    _packed("ends")
    _ranges("ends")
