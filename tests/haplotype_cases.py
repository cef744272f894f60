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


def piece_plan_rl(job):
    """piece_plan() with every piece walked in run-length form (cc.piece_runs) and its sums taken in Python integers: for CIGARs whose ops
    np.repeat cannot hold. The same return."""
    n_pieces = int(job["piece_off"][-1])
    plan, bundle = np.zeros((n_pieces, 4), np.int32), np.zeros(n_pieces, np.int64)
    for b in range(len(job["backbone_off"]) - 1):
        L = int(job["backbone_off"][b + 1] - job["backbone_off"][b])
        for p in range(int(job["piece_off"][b]), int(job["piece_off"][b + 1])):
            bundle[p] = b
            w = [int(x) for x in job["cigar"][job["cig_off"][p]:job["cig_off"][p + 1]]]
            ln, op = [x >> 4 for x in w], [x & 15 for x in w]
            n_bases = int(job["base_off"][p + 1] - job["base_off"][p])
            s = int(job["piece_sam_pos"][p])
            rd = sum(n for n, c in zip(ln, op) if c in (0, 1))
            if rd + sum(n for n, c in zip(ln, op) if c in (0, 2)) > INT32_MAX:
                plan[p] = (1, 1, 0, 0)
            elif n_bases == 0 or (int(job["piece_flags"][p]) & cc.START_BEYOND_SEQ) or rd != n_bases or s - 1 >= L:
                plan[p] = (1, 0, 0, 0)
            else:
                runs, ins = cc.piece_runs(ln, op, s, L)
                plan[p] = (0, 0, sum(r[1] for r in runs), len(ins))
    return plan, bundle


# ---- the limits: op lengths of 2^16 and more, and the refusal at 2^31 - 1 ------------------------------------------------------------------
# Where a case aims (the line a failure points to) is its `aim`. K = hs_kernels_consensus.hip, C = hs_capi_consensus.inc, R = hs_capi_refine.inc.
W28 = (1 << 28) - 1      # the longest op a CIGAR word holds
LADDER = (65535, 65536, 65537, W28)
LONG_L = 65600


def _limit(name, L, ops, T, Q, aim, at=0, n=3, text=None, flags=0, claim=None, plan=None, seed=None):
    """A bundle of n identical pieces walking `ops` from column `at` of a backbone of L columns. T, Q: what the M and D lengths and the M and I
    lengths must sum to, stated by the case and asserted here in Python integers, with T + Q: a case that lost its shape fails on the CPU.
    plan: the plan of one piece as the case claims it."""
    t, q = sum(k for k, c in ops if c in "MD"), sum(k for k, c in ops if c in "MI")
    assert (t, q, t + q) == (T, Q, T + Q) and all(0 <= k <= W28 for k, _ in ops), (name, t, q)
    bb = cc.seq(L, seed if seed is not None else L)
    if text is None:
        text, _ = cc._follow(bb, ops, at)
    b = cc.Bundle(name, bb, [(at + 1, [(k << 4) | cc.OPS.index(c) for k, c in ops], text, flags)] * n, claim=claim)
    b.aim, b.sums, b.plan = aim, (T, Q), plan
    return b, bb


def _good(L=40, seed=None, n=3):
    """a plain bundle: n pieces over all of the backbone, a substitution at column 3"""
    bb = cc.seq(L, seed if seed is not None else L)
    text = cc._sub(bb, 3, cc.other(bb[3]))
    b = cc.Bundle("a good bundle", bb, [(1, "%dM" % L, text)] * n, claim={"n_sub": 1, "n_skipped": 0, "cons": text})
    b.aim, b.sums, b.plan = "", (L, L), (0, 0, L, 0)
    return b


def length_cases():
    """One D op of 65535, 65536, 65537 and 2^28 - 1 events that overruns L = 40.
    Behind 10M: the columns from 10 on are deleted and n_cols is the room. K:93-94 (the two halves of wave_scan_incl_i64 and the shift that joins
    them), K:141 (n_cols = min(T, room) in 64 bits); in k_cons_rows K:47-48 (the int scans), K:65-66 (E and end), K:72 (T + v <= e).
    As the piece's FIRST column op, from s0 = 7: K:121 (col_ex = T + col_inc - a_col of lane 0), K:108 (room = L - s0), K:66."""
    out = []
    for n in LADDER:
        b, bb = _limit("10M %dD over L = 40" % n, 40, [(10, "M"), (n, "D")], 10 + n, 10, "K:93-94 K:141; rows K:47-48 K:65-66 K:72", plan=(0, 0, 40, 0), seed=n % 1000)
        b.claim = {"n_del": 30, "n_low": 0, "n_skipped": 0, "n_ins_bases": 0, "n_sub": 0, "cons": bb[:10]}
        out.append(b)
    for n in LADDER:
        b, bb = _limit("%dD 3M from s0 = 7" % n, 40, [(n, "D"), (3, "M")], n + 3, 3, "K:121 K:108; rows K:66", at=7, plan=(0, 0, 33, 0), seed=n % 1000 + 1)
        b.claim = {"n_del": 33, "n_low": 7, "n_skipped": 0, "n_ins_bases": 0, "cons": bb[:7]}
        out.append(b)
    return out


def long_m_cases():
    """L above 2^16, so that a column op can BEGIN at col_ex >= 2^16 inside the room.
    Long M, 10M 70000I 65536M 134217728D over L = 65600: an insertion capped at max_ins (K:60 cons_ins_cap, src = rd_ex - ins_before), the read
    cursor's high half (K:120 rd_inc, K:134 Q), an M op whose 65536 events run the 64-event loop of k_cons_rows 1024 times in one lane (K:67-79,
    txt[j_rd + off] with j_rd = 70010), 54 columns deleted behind it.
    Late insertion, ... 65536M 2I 5M inside L = 65600: the column op the 2I votes at begins at col_ex = 65546 (K:127 `col_ex < room` in 64 bits,
    K:55 `col_ex < pc.n_cols`, K:60 slot). Late overrun: the same CIGAR over L = 65546 -- that column op begins at col_ex = room: no vote."""
    ops = [(10, "M"), (70000, "I"), (65536, "M")]
    g32 = "G" * 32
    a, bb = _limit("long M: 10M 70000I 65536M 134217728D", LONG_L, ops + [(1 << 27, "D")], 10 + 65536 + (1 << 27), 10 + 70000 + 65536, "K:120 K:134 K:60; rows K:67-79",
                   plan=(0, 0, LONG_L, 1), seed=1)
    a.claim = {"n_ins_bases": 32, "n_del": LONG_L - 65546, "n_sub": 0, "n_low": 0, "n_skipped": 0, "cons": bb[:10] + g32 + bb[10:65546]}
    b, bb = _limit("late insertion: ... 65536M 2I 5M inside L", LONG_L, ops + [(2, "I"), (5, "M")], 65551, 135553, "K:127 K:55 K:60", plan=(0, 0, 65551, 2), seed=2)
    b.claim = {"n_ins_bases": 34, "n_del": 0, "n_sub": 0, "n_low": LONG_L - 65551, "n_skipped": 0, "cons": bb[:10] + g32 + bb[10:65546] + "GG" + bb[65546:]}
    c, bb = _limit("late overrun: ... 65536M 2I 5M, the 5M at col_ex = room", 65546, ops + [(2, "I"), (5, "M")], 65551, 135553, "K:127 K:55", plan=(0, 0, 65546, 1), seed=3)
    c.claim = {"n_ins_bases": 32, "n_del": 0, "n_sub": 0, "n_low": 0, "n_skipped": 0, "cons": bb[:10] + g32 + bb[10:]}
    return [a, b, c]


def chunk_cases():
    """A chunk whose 64 lanes all hold an op.
    Full chunk, 5M and 63 D ops of 2^25: every lane carries a high half, the low-half scan is all zeros but for lane 0 (K:93-94); T = 63 * 2^25 + 5
    stays below 2^31 and so inside the int scan of k_cons_rows (K:47). Mixed chunk: lengths 2^25 - 1 and 65537 alternate, both halves carry.
    Inert ops: twenty ops of 2^28 - 1 events, N = X P S H in turn, between 5M and 2I 35M: they count toward nothing (hs::cons_col_advance,
    hs::cons_read_advance; K:137 T + Q), the piece is accepted and its insertion votes at column 5 (K:125-127 across inert lanes)."""
    full = [(5, "M")] + [(1 << 25, "D")] * 63
    a, bb = _limit("full chunk: 5M and 63 x 33554432D", 40, full, 63 * (1 << 25) + 5, 5, "K:93-94; rows K:47", plan=(0, 0, 40, 0), seed=11)
    a.claim = {"n_del": 35, "n_low": 0, "n_skipped": 0, "cons": bb[:5]}
    mixed = [(5, "M")] + [((1 << 25) - 1 if i % 2 == 0 else 65537, "D") for i in range(63)]
    b, bb = _limit("mixed chunk: 5M, 33554431D and 65537D in turn", 40, mixed, 5 + 32 * ((1 << 25) - 1) + 31 * 65537, 5, "K:93-94 (a carry out of the low half)",
                   plan=(0, 0, 40, 0), seed=12)
    assert b.sums[0] == 1075773444
    b.claim = {"n_del": 35, "n_low": 0, "n_skipped": 0, "cons": bb[:5]}
    inert = [(5, "M")] + [(W28, "N=XPSH"[i % 6]) for i in range(20)] + [(2, "I"), (35, "M")]
    c, bb = _limit("inert ops: 20 x 268435455 of N = X P S H", 40, inert, 40, 42, "K:137 K:125-127", plan=(0, 0, 40, 1), seed=13)
    c.claim = {"n_ins_bases": 2, "n_sub": 0, "n_del": 0, "n_low": 0, "n_skipped": 0, "cons": bb[:5] + "GG" + bb[5:]}
    return [a, b, c]


AT_LIMIT = [(5, "M")] + [(W28, "D")] * 7 + [(268435452, "D")]       # T + Q = 2^31 - 1: T = 2147483642, Q = 5
OVER_LIMIT = [(5, "M")] + [(W28, "D")] * 7 + [(268435453, "D")]     # one more deleted base: T + Q = 2^31
MI_AT_LIMIT = [(W28, "M")] * 4 + [(3, "M"), (1, "I")]               # an M op counts twice, in T and in Q: T = 2^30 - 1, Q = 2^30
MI_OVER_LIMIT = [(W28, "M")] * 4 + [(3, "M"), (2, "I")]             # T = 2^30 - 1, Q = 2^30 + 1
FULL_AT_LIMIT = [(5, "M")] + [(1 << 25, "D")] * 62 + [(67108853, "D")]      # the limit again, every one of 64 lanes adding to it: T = 2147483642, Q = 5
FULL_OVER_LIMIT = [(5, "M")] + [(1 << 25, "D")] * 62 + [(67108854, "D")]


def boundary_cases():
    """T + Q = 2^31 - 1 exactly: accepted (K:137 `T + Q > 0x7fffffff`, hs_consensus_host.h cons_piece_plan `all > 0x7fffffff`; C:177, C:324).
    With D ops, in 9 lanes and in all 64 of a chunk: the plan is (0, 0, room, 0) and the deletions win. With M and I ops against a text of four bases -- an M op counts twice, once
    in T and once in Q -- the piece is not long and therefore skipped for its base count (K:138), beside three good pieces."""
    a, bb = _limit("at the limit: 5M, 7 x 268435455D, 268435452D", 40, AT_LIMIT, 2147483642, 5, "K:137 C:177 C:324; rows K:47 K:65", plan=(0, 0, 40, 0), seed=21)
    a.claim = {"n_del": 35, "n_low": 0, "n_skipped": 0, "n_ins_bases": 0, "cons": bb[:5]}
    c, bb = _limit("at the limit, a full chunk: 5M, 62 x 33554432D, 67108853D", 40, FULL_AT_LIMIT, 2147483642, 5, "K:93-94 K:134 K:137 (the sum of 64 lanes, to the base)",
                   plan=(0, 0, 40, 0), seed=23)
    c.claim = {"n_del": 35, "n_low": 0, "n_skipped": 0, "n_ins_bases": 0, "cons": bb[:5]}
    g = _good(seed=22)
    b, _ = _limit("at the limit, M and I form: 4 x 268435455M 3M 1I", 40, MI_AT_LIMIT, (1 << 30) - 1, 1 << 30, "K:137 K:138", text="ACGT", n=1, plan=(1, 0, 0, 0), seed=22)
    b.pieces = g.pieces + b.pieces
    b.claim = dict(g.claim, n_skipped=1)
    return [a, b, c]


LIMIT_CASES = {"lengths": length_cases, "long_m": long_m_cases, "chunks": chunk_cases, "boundary": boundary_cases}


def _over(ops=OVER_LIMIT, text=None, flags=0, n=1):
    T, Q = sum(k for k, c in ops if c in "MD"), sum(k for k, c in ops if c in "MI")
    assert T + Q == 1 << 31
    return _limit("over the limit", 40, ops, T, Q, "K:137 K:143", text=text, flags=flags, n=n, plan=(1, 1, 0, 0), seed=30)[0].pieces


def refused_cases():
    """T + Q = 2^31: the whole call is refused with "bundle b: a CIGAR of more than 2^31 - 1 bases" -- refused, not skipped -- by the host half
    (hs_consensus_host.cpp:149), by the host-planned route (C:177) and from the device's flag (K:143 the atomic minimum, C:301 its start value,
    C:321-328 the bundle it names; R:204-208 behind a pass). [(name, bundles, the bundle the message names)], varying where the long piece sits."""
    good = _good(seed=31).pieces
    with_long = lambda pieces: cc.Bundle("a bundle with a long piece", cc.seq(40, 30), pieces)
    return [
        ("the only piece", [with_long(_over())], 0),
        ("piece 5 of its bundle: the second workgroup of k_cons_plan", [with_long(good + good[:2] + _over() + good[:2])], 0),
        ("in bundle 2 of 3", [_good(seed=32), _good(seed=33), with_long(good[:1] + _over() + good[:1])], 2),
        ("two long pieces, in the bundles 1 and 2: the lower one is named", [_good(seed=32), with_long(good + _over()), with_long(_over() + good)], 1),
        ("a long piece with empty text: long first", [_good(seed=32), with_long(good + _over(text=""))], 1),
        ("a long piece flagged START_BEYOND_SEQ: long first", [with_long(good + _over(flags=cc.START_BEYOND_SEQ))], 0),
        ("M and I form, against four bases: long first, its base count second", [_good(seed=32), with_long(good + _over(MI_OVER_LIMIT, text="ACGT"))], 1),
        ("a full chunk of 64 ops, one base over", [with_long(good + _over(FULL_OVER_LIMIT))], 0),
    ]


def check_limit_plan(bundles, plan):
    """the plan every case claims for its pieces (b.plan: of the LAST pieces of the bundle where good ones stand in front), and the good ones'"""
    p = 0
    for b in bundles:
        for i in range(len(b.pieces)):
            own = b.plan if (b.plan[0] == 0 or i == len(b.pieces) - 1) else (0, 0, len(b.backbone), 0)
            assert tuple(int(x) for x in plan[p]) == tuple(own), (b.name, b.aim, i, plan[p].tolist(), own)
            p += 1
