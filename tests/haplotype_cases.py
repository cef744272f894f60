"""The plan of a piece on the device (k_cons_plan) and the call from labels to haplotype sequences: the shapes at which a chunked,
wave-parallel plan can differ from the sequential one (hs::cons_piece_plan), as bundles of tests/consensus_cases.py, and a numpy restatement of
the plan. A case has three identical pieces unless its name says otherwise; its `claim` is worked out by hand from the rule. Ops are numbered
from 0: a wavefront reads the ops 0..63 in its first chunk, 64..127 in its second."""
import numpy as np

import consensus_cases as cc

INT32_MAX = 0x7FFFFFFF


def _bundle(name, L, ops, at=0, n=3, seed=None, claim=None, text=None):
    bb = cc.seq(L, seed if seed is not None else L)
    follow, _ = cc._follow(bb, ops, at)
    w = [(k << 4) | cc.OPS.index(c) for k, c in ops]
    return cc.Bundle(name, bb, [(at + 1, w, follow if text is None else text)] * n, claim=claim), bb


def chunk_edge_cases():
    out = []
    for edge in (63, 127):      # the insertion is the chunk's last op, the column op it votes at the next chunk's first
        b, bb = _bundle("op %d is I, op %d is M" % (edge, edge + 1), edge + 17, [(1, "M")] * edge + [(2, "I"), (5, "M")])
        b.claim = {"n_ins_bases": 2, "n_skipped": 0, "n_low": 12, "cons": bb[:edge] + "GG" + bb[edge:]}
        out.append(b)
    b, bb = _bundle("ops 63 and 64 are I, op 65 is M", 80, [(1, "M")] * 63 + [(1, "I"), (2, "I"), (5, "M")])
    b.claim = {"n_ins_bases": 3, "n_skipped": 0, "cons": bb[:63] + "GGG" + bb[63:]}
    out.append(b)
    b, bb = _bundle("ops 62 I, 63 0M, 64 I, 65 M", 80, [(1, "M")] * 62 + [(1, "I"), (0, "M"), (2, "I"), (4, "M")])
    b.claim = {"n_ins_bases": 3, "n_skipped": 0, "cons": bb[:62] + "GGG" + bb[62:]}
    out.append(b)
    b, bb = _bundle("64 inert ops, then I, then M", 12, [(1, "=XNP"[i % 4]) for i in range(64)] + [(2, "I"), (10, "M")])
    b.claim = {"n_ins_bases": 0, "n_skipped": 0, "n_low": 2, "cons": bb}
    out.append(b)
    return out


def room_cases():
    out = []
    L = 40
    b, bb = _bundle("M ends on column L - 1, then I M", L, [(L, "M"), (2, "I"), (3, "M")])
    b.claim = {"n_ins_bases": 0, "n_skipped": 0, "n_low": 0, "cons": bb}
    out.append(b)
    b, bb = _bundle("M ends on column L - 2, then I M", L, [(L - 1, "M"), (2, "I"), (3, "M")])
    b.claim = {"n_ins_bases": 2, "n_skipped": 0, "n_low": 0, "cons": bb[:L - 1] + "GG" + bb[L - 1:]}
    out.append(b)
    # 130 ops: 70 M, then 30 (I, M) pairs; the insertion of pair i lies in front of column 70 + i, and the room is 80 columns
    b, bb = _bundle("130 ops, the room ends inside chunk 2", 80, [(1, "M")] * 70 + [(1, "I"), (1, "M")] * 30)
    b.claim = {"n_ins_bases": 10, "n_skipped": 0, "n_low": 0, "cons": bb[:70] + "".join("G" + bb[70 + i] for i in range(10))}
    out.append(b)
    return out


def skip_cases():
    ops = [(1, "M")] * 129 + [(2, "M")]      # 131 bases by the CIGAR; the text has the 130 that "1M" in place of op 129 would give
    bb = cc.seq(140, 140)
    b, _ = _bundle("130 ops, only op 129 makes the sum differ", 140, ops, text=bb[:130])
    b.claim = {"n_skipped": 3, "n_low": 140, "n_sub": 0, "cons": bb}
    good = lambda k: _bundle("whole bundle %d" % k, 20 + k, [(20 + k, "M")], seed=300 + k, claim={"n_skipped": 0, "n_low": 0})[0]
    bb2 = cc.seq(30, 31)
    dead = cc.Bundle("every piece skipped, between two bundles with none", bb2, [(1, "30M", ""), (1, "29M", bb2), (31, "1M", "A"), (1, "30M", bb2, cc.START_BEYOND_SEQ)],
                     claim={"n_skipped": 4, "n_low": 30, "cons": bb2})
    return [b, good(0), dead, good(1)]


def count_cases(n):
    """one bundle of n pieces: four wavefronts make a workgroup of k_cons_plan"""
    bb = cc.seq(24, 24 + n)
    text = cc._sub(bb, 5, cc.other(bb[5]))
    return [cc.Bundle("%d pieces in the call" % n, bb, [(1, "12M1I12M", text[:12] + "G" + text[12:])] * n,
                      claim={"n_skipped": 0, "n_sub": 1 if n >= cc.MIN_COV else 0, "n_ins_bases": 1 if n >= cc.MIN_COV else 0, "n_low": 0 if n >= cc.MIN_COV else 24})]


CASES = {"chunk_edges": chunk_edge_cases, "room": room_cases, "skip": skip_cases, "count0": lambda: count_cases(0), "count1": lambda: count_cases(1),
         "count4": lambda: count_cases(4), "count5": lambda: count_cases(5)}


def all_groups():
    """(name, bundles) of every group of consensus_cases.CASES and of CASES above"""
    return [("cc." + g, cc.CASES[g]()) for g in sorted(cc.CASES)] + [("hc." + g, CASES[g]()) for g in sorted(CASES)]


def piece_plan(job):
    """hs::cons_piece_plan restated from the rule's text (hs_consensus_host.h: walk, skipped pieces, slot): [n_pieces][4] = skipped, long_cigar,
    the columns the piece covers (clipped at L), the insertions that vote. And the bundle of every piece."""
    n_pieces = int(job["piece_off"][-1])
    plan, bundle = np.zeros((n_pieces, 4), np.int32), np.zeros(n_pieces, np.int64)
    for b in range(len(job["backbone_off"]) - 1):
        L = int(job["backbone_off"][b + 1] - job["backbone_off"][b])
        for p in range(int(job["piece_off"][b]), int(job["piece_off"][b + 1])):
            bundle[p] = b
            w = job["cigar"][job["cig_off"][p]:job["cig_off"][p + 1]].astype(np.int64)
            ln, op = w >> 4, w & 15
            n_bases = int(job["base_off"][p + 1] - job["base_off"][p])
            s = int(job["piece_sam_pos"][p])
            rd = int(ln[(op == 0) | (op == 1)].sum())
            if rd + int(ln[(op == 0) | (op == 2)].sum()) > INT32_MAX:
                plan[p] = (1, 1, 0, 0)
                continue
            if n_bases == 0 or (int(job["piece_flags"][p]) & cc.START_BEYOND_SEQ) or rd != n_bases or s - 1 >= L:
                plan[p] = (1, 0, 0, 0)
                continue
            ev = np.repeat(op, ln)
            ev = ev[ev <= 2]                       # one entry per M, I or D char
            is_col = ev != 1
            t = s - 1 + np.cumsum(is_col) - is_col
            ce = np.flatnonzero(is_col & (t < L))  # the column events of the walk: it ends at the first t >= L
            n_ins = int((np.diff(ce) > 1).sum())   # between two column events there are only I chars: an insertion of the piece, in the later one's slot
            plan[p] = (0, 0, len(ce), n_ins)
    return plan, bundle
