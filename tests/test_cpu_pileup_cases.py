"""The cases of tests/pileup_cases.py are what they claim to be, shown with the oracle and numpy alone (no GPU): every fork counter a case claims is
reached (pileup_cases.analyse), the three constants of the decomposition are the kernel's, a plain per-event walk of the records equals the oracle's
generate_msa byte for byte and counter for counter, and the same walk with one deliberate defect at a time differs from the oracle on the case that claims the
fork -- so tests/test_gpu_pileup_cases.py, which holds the device to the same oracle, would see a kernel with that defect."""
import collections
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import pileup_cases as pc


@pytest.fixture(scope="module", autouse=True)
def _artefacts(built):
    return built


_memo = {}


def load(name):
    """(flat batch, analysis, the oracle's pile, the oracle's stats) of a case, computed once"""
    if name not in _memo:
        from hairsplitter_amd import api
        flat = api.FlatBatch(pc.get(name))
        pile, stats, _ = ol.pileup(flat)
        pile.setflags(write=False); stats.setflags(write=False)
        _memo[name] = (flat, pc.analyse(flat), pile, stats)
    return _memo[name]


def walk(flat, defect=None):
    """generate_msa (call_variants.cpp:189-354) event by event: the pile in the packed layout and (q_end, n_err, n_len) per record. Knows nothing of chunks,
    tasks or pieces -- except where `defect` names a way the run form could go wrong."""
    pile = np.zeros(flat.aligned_bp, np.uint8); stats = np.zeros((flat.n_rec, 3), np.int32)
    for r in range(flat.n_rec):
        c = int(flat.rec_contig[r]); seq = flat.contig_seq[int(flat.contig_off[c]):int(flat.contig_off[c + 1])]; L = len(seq)
        rd = int(flat.rec_read[r]); read = flat.read_seq[int(flat.read_off[rd]):int(flat.read_off[rd + 1])]
        if not flat.rec_strand[r]:
            read = 3 - read[::-1]
        pos = q = int(flat.rec_pos[r]); t = 0; p1, p2 = 2, 1; nerr = nlen = 0; last_ev = 0      # 'G', 'C' (call_variants.cpp:212-214)
        for oi, w in enumerate(flat.cigar[int(flat.rec_cig_off[r]):int(flat.rec_cig_off[r + 1])]):
            n, op = int(w) >> 4, int(w) & 15
            if defect == "reset_at_op_128" and oi == 128: p1, p2 = 2, 1
            if defect == "single_event_op_supplies_both" and oi and oi % 64 == 0 and last_ev == 1: p2 = p1
            if defect == "zero_event_ops_reset" and (n == 0 or op in (pc.N, pc.P)): p1, p2 = 2, 1
            if defect == "insertion_at_L_counted" and op == pc.I and q == L: nerr += n; nlen += n
            for j in range(n):
                if not q < L:
                    if defect == "cut_op_counts_whole_piece" and op in (pc.M, pc.EQ, pc.X, pc.D) and j % 16: nlen += min(16 - j % 16, n - j)
                    break
                if op in (pc.S, pc.H): t += 1; continue
                if op in (pc.N, pc.P): break
                if defect == "deletion_piece_context_from_read" and op == pc.D and j and j % 16 == 0: p1, p2 = int(read[t - 1]), int(read[t - 2])
                ch = 4 if op == pc.D else int(read[t])
                if op != pc.I:
                    pile[int(flat.pile_off[r]) + q - pos] = 33 + 25 * ch + p1 + 5 * p2
                    nerr += ch != seq[q]; q += 1
                else: nerr += 1
                if op != pc.D: t += 1
                nlen += 1; p2, p1 = p1, ch
            if n and op in (pc.M, pc.EQ, pc.X, pc.D, pc.I): last_ev = n
        stats[r] = (q, nerr, nlen)
    return pile, stats


# the defect -> the case whose forks it hangs on
DEFECTS = {"deletion_piece_context_from_read": "pieces", "reset_at_op_128": "boundaries", "single_event_op_supplies_both": "boundaries", "zero_event_ops_reset": "context",
           "insertion_at_L_counted": "pieces", "cut_op_counts_whole_piece": "pieces"}


def _check(name):
    flat, an, o_pile, o_stats = load(name)
    missing = [f for f in pc.FORKS[name] if an.forks[f] < 1]
    assert not missing, (name, missing)
    assert len(o_pile) == 0 or (33 <= int(o_pile.min()) and int(o_pile.max()) <= 157)
    assert np.array_equal(o_stats[:, 2], an.n_on_contig)
    pile, stats = walk(flat)
    assert np.array_equal(pile, o_pile)
    assert np.array_equal(stats, o_stats[:, :3])
    assert flat.n_contigs <= 6 and flat.n_rec <= 400 and int(np.diff(flat.contig_off).max()) <= 10_000
    for defect, case in DEFECTS.items():
        if case == name:
            d_pile, d_stats = walk(flat, defect)
            assert not (np.array_equal(d_pile, o_pile) and np.array_equal(d_stats, o_stats[:, :3])), defect
    print(name, flat.n_rec, "records;", {k: an.forks[k] for k in pc.FORKS[name]})
    return an


def test_constants_are_the_kernels():
    src = open(os.path.join(ol.ROOT, "hairsplitter_amd", "csrc", "hs_kernels_runs.inc")).read()
    got = {k: int(re.search(rf"^#define {k} (\d+)", src, re.M).group(1)) for k in ("HS_K1R_PIECE", "HS_K1R_MAPW", "HS_K1R_NCH")}
    assert got == {"HS_K1R_PIECE": pc.PIECE, "HS_K1R_MAPW": pc.MAPW, "HS_K1R_NCH": pc.NCH}


def test_context():
    """all 14 (last event, event before, op kind) combinations inside one chunk, plain and with N / P / 0M / 0D / 0I in between, on both strands"""
    _check("context")


def test_boundaries():
    """the same combinations with the op at index 64, 128 and 256; K0's three ways over a chunk edge; K1's five sources for the two events before an op"""
    an = _check("boundaries")
    assert not load("boundaries")[1].flagged.any()
    assert (an.chunk_table[:, 3] >> 4).max() <= 15


def test_pieces():
    """tails of 1 .. 15 events and contig cuts at 0 .. 15 events, for M-like and D pieces on both strands; second and third pieces of a deletion"""
    _check("pieces")


def test_windows():
    """tasks of 0, 255, 256, 257, 512, 513 pieces; ops that start at piece 255 and 256; M and D ops of more than 512 pieces; a task beyond the contig end"""
    _check("windows")


def test_flags():
    """K0's rule for the records that are not one run of events, either side of it"""
    an = _check("flags")
    flat = load("flags")[0]
    assert 0 < int(an.flagged.sum()) < flat.n_rec


def test_ends():
    """records at L - 1, L and L + 5, without ops, of clips only; contigs of 1, 2, 3 and 17 bases and one without records"""
    _check("ends")


def test_every_fork_is_reached_by_some_case():
    reached = collections.Counter()
    for name in pc.NAMES:
        reached.update(load(name)[1].forks)
    need = [f"ctx:{at}:{c}:{s}" for at in ("in", "e64", "e128", "e256") for c in pc.ALL_CTX for s in "fr"]
    need += [f"{what}:{k}:{n}:{s}" for what, lo in (("tail", 1), ("cut", 0)) for k in "MD" for n in range(lo, 16) for s in "fr"]
    need += [f for name in ("windows", "flags", "ends") for f in pc.FORKS[name]]
    assert len(need) == 2 * (4 * 14 + 2 * 15 + 2 * 16) + sum(len(pc.FORKS[n]) for n in ("windows", "flags", "ends"))
    assert not [f for f in need if reached[f] < 1]
    assert set(DEFECTS.values()) <= set(pc.NAMES)      # every defect is tried by the test of its case
