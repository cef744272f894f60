"""Alignment records for the pileup front of stage 3 -- K0 k_cigar_scan (hs_kernels.hip) and K1 k_pileup_runs (hs_kernels_runs.inc) with
k_pileup_flagged_records -- built from explicit CIGAR arrays at every fork of the run form's decomposition: the 14 contexts of an op's first column, inside
a chunk and across the chunk and task edges; pieces of every length, cut by the op and by the contig end; windows of 256 pieces either side of their
limits; K0's rule for the records the run form leaves out; degenerate records and contigs. Used by tests/test_cpu_pileup_cases.py (which proves with the
oracle alone that every case reaches the forks it claims) and tests/test_gpu_pileup_cases.py.

A case is a list of synth.ContigData; read bases are seeded; a read is as long as its CIGAR consumes unless the record says otherwise (`rlen`).
analyse(flat) restates ONLY the decomposition (which op lands in which chunk, task, piece and window, and where its context comes from): never a code."""
import collections
import types

import numpy as np

# ---- the three constants the decomposition hangs on (tests/test_cpu_pileup_cases.py compares them with the #defines of hs_kernels_runs.inc) ----
PIECE = 16      # HS_K1R_PIECE: events of one M / = / X / D op a lane takes
MAPW = 256      # HS_K1R_MAPW: pieces per window of the piece -> op map
NCH = 2         # HS_K1R_NCH: 64-op chunks of K0's table per run-form task
CHUNK = 64      # ops per entry of K0's table (one wavefront, lane = op)
TASK_OPS = CHUNK * NCH

M, I, D, N, S, H, P, EQ, X = range(9)      # BAM op codes (synth.OP_*)
_MLIKE = (M, EQ, X)
_KIND = {M: "M", EQ: "M", X: "M", D: "D"}
CONTEXTS = ((2, 3), (0, 2), (1, 2), (0, 0), (0, 1), (1, 0), (1, 1))      # (type of the last event, of the one before): 0 read base, 1 deletion, 2 / 3 none yet
EDGES = {CHUNK: "e64", TASK_OPS: "e128", 2 * TASK_OPS: "e256"}
ZERO_OPS = ((7, N), (3, P), (0, M), (0, D), (0, I))                      # ops without events that move no cursor


def _adv(n, o):
    """(events, read bases, contig bases) an op consumes: call_variants.cpp:226-342 (S and H step over read bases, N and P over nothing)"""
    return (n if o in _MLIKE or o in (I, D) else 0, n if o in _MLIKE or o in (I, S, H) else 0, n if o in _MLIKE or o == D else 0)


class _Case:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.contigs = []

    def contig(self, name, L, recs):
        """recs: (pos, forward, ops[, rlen]); every record brings its own read"""
        from hairsplitter_amd import synth
        seq = self.rng.integers(0, 4, size=L).astype(np.uint8)
        reads, names, alns = [], [], []
        for k, rec in enumerate(recs):
            pos, fwd, ops = rec[:3]
            rl = rec[3] if len(rec) > 3 else sum(_adv(n, o)[1] for n, o in ops)
            reads.append(self.rng.integers(0, 4, size=rl).astype(np.uint8))
            names.append(f"{name}_r{k}")
            alns.append(synth.Alignment(k, pos, fwd, np.array([(n << 4) | o for n, o in ops], dtype=np.uint32), 0))
        self.contigs.append(synth.ContigData(name, seq, reads, names, alns, np.zeros(len(recs), np.int32)))


def _both(recs):
    """every record on both strands, as sibling records of one call"""
    return [(r[0], fwd) + tuple(r[1:]) for r in recs for fwd in (True, False)]


# prefixes that leave each context in front of the next op (several per context: read bases by M, =, X and by I)
_PREFIX = {
    (2, 3): [[]],
    (0, 2): [[(1, M)], [(1, I)], [(1, X)]],
    (1, 2): [[(1, D)]],
    (0, 0): [[(5, M)], [(2, I)], [(3, I)], [(1, EQ), (1, X)], [(1, D), (1, I), (1, M)]],
    (0, 1): [[(3, M), (1, D), (1, M)], [(2, D), (1, I)], [(1, D), (1, EQ)]],
    (1, 0): [[(3, M), (1, D)], [(1, I), (1, D)], [(4, X), (1, D)]],
    (1, 1): [[(2, D)], [(4, M), (1, D), (2, D)], [(1, D), (1, D)], [(2, D), (2, D)]],
}
_TARGETS = [[(5, M)], [(3, D)], [(4, EQ)], [(2, X)]]      # the op whose first column takes the context (an M-like op or a D op), then a tail
_TAIL = [(4, M)]


def _with_zero_ops(prefix, k0=0):
    """the prefix with ops that own no event behind every op of it (and in front of an empty one)"""
    out, k = [], k0
    for op in prefix or [None]:
        if op is not None:
            out.append(op)
        out.append(ZERO_OPS[k % len(ZERO_OPS)]); k += 1
    out.append(ZERO_OPS[k % len(ZERO_OPS)])
    return out


def _context():
    cs = _Case(101)
    recs = []
    for ctx in CONTEXTS:
        for pi, prefix in enumerate(_PREFIX[ctx]):
            for ti, target in enumerate(_TARGETS):
                recs.append((len(recs) % 37, prefix + target + _TAIL))
                recs.append((len(recs) % 37, _with_zero_ops(prefix, pi + ti) + target + _TAIL))
    cs.contig("ctx", 160, _both(recs))
    return cs.contigs


_FILL = [(2, M), (1, D), (1, M), (1, I)]      # short ops with events, to move an op to a given index
_ZFILL = [(3, N), (2, P)]                     # and without


def _fill(n, pattern=_FILL, k0=0):
    return [pattern[(k0 + k) % len(pattern)] for k in range(n)]


def _placed(at, prefix, target, ctx):
    """`target` as op `at` of the record with `prefix` directly before it; the ops in front of the prefix own events unless the context needs a record
    with fewer than two events so far"""
    lead = at - len(prefix)
    assert lead >= 0
    return _fill(lead, _ZFILL if ctx[1] >= 2 else _FILL, at) + prefix + target + _fill(5) + _TAIL


def _boundaries():
    cs = _Case(102)
    recs = []
    for at in EDGES:
        for ci, ctx in enumerate(CONTEXTS):
            for ti, target in enumerate(_TARGETS[:2]):
                recs.append((len(recs) % 29, _placed(at, _PREFIX[ctx][(ci + ti) % len(_PREFIX[ctx])], target, ctx)))
    for target in _TARGETS[:2]:
        for last in ((1, D), (1, I)):
            # the last op of a chunk is the only op of its chunk with events (63 N / P ops in front of it): K0 keeps the event before it from the chunks below
            recs.append((3, _fill(CHUNK) + _fill(CHUNK - 1, _ZFILL) + [last] + target + _TAIL))
            recs.append((5, _fill(CHUNK - 1, _ZFILL) + [last] + target + _fill(CHUNK - 2) + [(3, M)] + target + _TAIL))
            recs.append((7, _fill(3 * CHUNK, k0=1) + _fill(CHUNK - 1, _ZFILL) + [last] + target + _TAIL))
        # a chunk of 64 ops without an event between two chunks that have events: at a chunk edge inside a task, at a task edge
        recs.append((2, _fill(CHUNK) + _fill(CHUNK, _ZFILL) + target + _fill(70) + _TAIL))
        recs.append((4, _fill(CHUNK, k0=2) + _fill(CHUNK, _ZFILL) + _fill(CHUNK, k0=1) + _fill(CHUNK, _ZFILL) + target + _TAIL))
        recs.append((6, _fill(2 * CHUNK, k0=3) + _fill(CHUNK, _ZFILL) + target + _fill(3) + target + _TAIL))
        # K1's search for the two events before an op inside its task
        recs.append((1, _fill(CHUNK) + [(1, I)] + target + _TAIL))                                # the last in the op's own chunk, the one before in the lower chunk
        recs.append((1, _fill(CHUNK, k0=1) + [(1, D), (3, N), (2, P)] + target + _TAIL))          # the same, ops without events in between
        recs.append((2, _fill(TASK_OPS) + [(1, M)] + target + _TAIL))                             # one found, the other from K0's entry
        recs.append((2, _fill(TASK_OPS, k0=1) + [(1, D), (0, M)] + target + _TAIL))
        recs.append((3, _fill(2 * TASK_OPS, k0=2) + [(1, I), (2, P)] + target + _TAIL))
        recs.append((3, _fill(TASK_OPS, k0=3) + [(3, N), (2, P), (0, M), (0, D), (0, I)] + target + _TAIL))      # none: the task's earlier ops own no event
        recs.append((4, _fill(TASK_OPS + CHUNK, k0=1) + target + _TAIL))                          # both in the lower chunk
    cs.contig("edges", 700, _both(recs))
    return cs.contigs


PIECE_LENGTHS = tuple(range(1, 18)) + (31, 32, 33, 40)


def _pieces():
    cs = _Case(103)
    recs = [(7 * k % 23, [(n, M), (n, D), (n, EQ), (1, I), (n, X), (2, M)]) for k, n in enumerate(PIECE_LENGTHS)]
    recs += [(11, [(k, S), (20, M)]) for k in range(4)] + [(13, [(k, I), (20, EQ)]) for k in range(1, 4)]      # the first column op at read offset 0 .. 3
    cs.contig("lengths", 230, _both(recs))
    cs.contig("tiny_reads", 40, [(n, False, [(n, M)]) for n in range(1, 16)] + [(3 + k, False, [(20, M), (k, S)]) for k in range(16)]
              + [(2, True, [(n, X)]) for n in range(1, 16)])
    L = 97
    recs = []
    for kind in (M, D):
        for k in range(16):      # the piece that holds the contig end keeps k events; one whole piece before it, one beyond
            recs.append((L - PIECE - k - 2, [(2, M), (40, kind)]))
    recs += [(L - 5, [(4, M), (1, I), (1, M)]), (L - 5, [(5, M), (2, I)]), (L - 3, [(3, EQ), (1, I), (4, M)])]      # an insertion at q == L - 1 and at q == L
    cut = _both(recs)
    # a CIGAR that consumes more bases than the read has, beyond the contig end only (hs_cv_batch_create tolerates it when pos + refspan > L)
    cut += [(L - 10, True, [(30, M)], 15), (L - 10, False, [(30, M)], 15), (L - 20, True, [(18, M), (2, D), (3, I), (40, EQ)], 23),
            (L - 20, False, [(18, M), (2, D), (3, I), (40, EQ)], 23)]
    cs.contig("cut", L, cut)
    return cs.contigs


def _np_ops(parts, tail=5):
    """M ops of 16 p events for p in parts (the last one `tail` events short), an insertion between them: sum(parts) pieces"""
    ops = []
    for k, p in enumerate(parts):
        if k:
            ops.append((1, I))
        ops.append((PIECE * p - (tail if k == len(parts) - 1 else 0), (M, EQ, X)[k % 3]))
    return ops


def _windows():
    cs = _Case(104)
    L = 9000
    recs = [(10 * k, _np_ops(parts)) for k, parts in enumerate(([200, 55], [200, 56], [200, 57], [300, 212], [300, 213], [100, 28], [100, 29], [255, 10],
                                                                 [100, 156, 10], [1, 514], [512, 3]))]
    recs.append((20, [(3, M), (PIECE * 513 + 2, D), (5, M)]))                    # a D op of 514 pieces behind a column op
    recs.append((30, _fill(TASK_OPS, [(1, I), (3, N), (2, P), (0, M)]) + [(50, M), (2, D), (20, M)]))      # a task without a piece, then one with pieces
    recs.append((L - 100, _fill(TASK_OPS, [(2, M), (1, D)]) + _fill(40, [(1, M), (1, I), (17, D)]) + [(33, M)]))      # the second task lies beyond the contig end
    cs.contig("win", L, _both(recs))
    return cs.contigs


def _flags():
    cs = _Case(105)
    recs = []
    for clip in (S, H):
        recs.append((3, [(10, M), (5, clip), (10, M)]))
        recs.append((5, _fill(CHUNK, [(1, M), (1, I)]) + [(5, clip)] + _fill(CHUNK - 1, _ZFILL) + [(10, M)]))      # the clip at op 64, events in chunks 0 and 2 only
        recs.append((7, _fill(CHUNK) + [(4, clip)] + _fill(70)))                                                  # events before it in the chunk below, after it in its own
        recs.append((9, [(10, M), (5, clip), (2, P), (2, P)]))                                                    # events before, none after: the run form
        recs.append((11, [(5, clip), (3, H), (3, N), (0, M), (10, M)]))                                           # leading clips, then ops without events
        recs.append((13, [(10, M), (100, clip), (10, EQ), (2, D), (3, M)]))                                       # a clip longer than 64 events' worth of read
        recs.append((15, [(100, clip), (10, M), (1, I), (30, M)]))
        recs.append((2, _fill(140, [(1, M), (1, I)]) + [(3, clip)] + _fill(200, [(2, M), (1, D)])))               # flagged, 341 ops: tasks at k = 0, 2, 4
    recs.append((17, [(5, M), (7, N), (5, M), (2, P), (2, D), (3, M)]))                                           # N / P between events: one run of events
    recs.append((1, _fill(300)))                                                                                  # as long, not flagged
    cs.contig("flags", 420, _both(recs))
    return cs.contigs


def _ends():
    cs = _Case(106)
    L = 17
    recs = [(0, [(17, M)]), (L - 1, [(1, M)]), (L - 1, [(3, M)]), (L - 1, [(1, D), (2, M)]), (L, [(5, M)]), (L, [(2, D), (1, I)]), (L + 5, [(5, M), (1, D)]),
            (2, [(4, M)]), (3, []), (4, [(3, M), (1, D), (2, M)]), (5, [(5, S)]), (6, [(3, H), (2, S)]), (0, [(2, I), (16, M)])]
    cs.contig("L17", L, _both(recs))
    cs.contig("L1", 1, _both([(0, [(1, M)]), (0, [(1, D)]), (0, [(1, I), (1, M)]), (0, [(2, D)]), (1, [(1, M)])]))
    cs.contig("none", 40, [])
    cs.contig("L2", 2, _both([(0, [(2, M)]), (1, [(1, X)]), (0, [(1, D), (1, M)]), (0, [(3, M)])]))
    cs.contig("L3", 3, _both([(0, [(3, EQ)]), (1, [(1, M), (1, I), (1, M)]), (2, [(1, M)]), (0, [(1, M), (5, D)])]))
    return cs.contigs


_CASES = {"context": _context, "boundaries": _boundaries, "pieces": _pieces, "windows": _windows, "flags": _flags, "ends": _ends}
NAMES = tuple(_CASES)
_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = _CASES[name]()
    return _cache[name]


# ------------------------------------------------------------------------------------------------
# the decomposition, restated
# ------------------------------------------------------------------------------------------------
def _ctx_name(ctx, kind):
    return f"{ctx[0]}{ctx[1]}{kind}"


def analyse(flat):
    """What K0 and the run form of K1 make of every record of the batch, in plain Python. Returns a namespace:
    forks        Counter of named forks (see FORKS)
    chunk_table  int32 [n_chunks, 4]: K0's table (hs_kernels.hip, k_cigar_scan): per 64-op chunk the events, read bases and the contig cursor before it, and
                 (ctx1 | ctx2 << 2) << 4, bit 0 set on the first chunk of a record that is not one run of events
    chunk_off    int64 [n_rec + 1]
    flagged      bool [n_rec]
    n_events     int64 [n_rec] events of the CIGAR; n_on_contig: those on the contig (what n_len counts)"""
    forks = collections.Counter()
    n_rec = flat.n_rec
    lens = np.diff(flat.contig_off)
    table, chunk_off = [], [0]
    flagged = np.zeros(n_rec, bool); n_events = np.zeros(n_rec, np.int64); n_on = np.zeros(n_rec, np.int64)
    for c in range(flat.n_contigs):
        r0, r1 = int(flat.contig_rec_off[c]), int(flat.contig_rec_off[c + 1])
        if r1 > r0 and int(lens[c]) in (1, 2, 3, 17):
            forks[f"end:L={int(lens[c])}"] += 1
        if r1 == r0 and 0 < c < flat.n_contigs - 1 and flat.contig_rec_off[c] > 0 and flat.contig_rec_off[-1] > r1:
            forks["end:contig_without_records_between"] += 1
    for r in range(n_rec):
        c = int(flat.rec_contig[r]); L = int(lens[c]); pos = int(flat.rec_pos[r]); s = "f" if flat.rec_strand[r] else "r"
        rd_i = int(flat.rec_read[r]); rlen = int(flat.read_off[rd_i + 1] - flat.read_off[rd_i])
        ops = [(int(w) >> 4, int(w) & 15) for w in flat.cigar[int(flat.rec_cig_off[r]):int(flat.rec_cig_off[r + 1])]]
        n_ops = len(ops)
        adv = [_adv(n, o) for n, o in ops]
        e0, t0, q0, ctx = [0], [0], [pos], [(2, 3)]      # before op i: events, read cursor, contig cursor, the two events before
        for (n, o), (ev, rd, rf) in zip(ops, adv):
            e0.append(e0[-1] + ev); t0.append(t0[-1] + rd); q0.append(q0[-1] + rf)
            c1, c2 = ctx[-1]
            ty = 1 if o == D else 0
            ctx.append((c1, c2) if ev == 0 else ((ty, c1) if ev == 1 else (ty, ty)))
        total = e0[-1]
        n_events[r] = total
        # ---- K0: a clip with events before it and after it ----
        gaps = [i for i in range(n_ops) if adv[i][0] == 0 and (adv[i][1] > 0 or adv[i][2] > 0)]
        flg = any(0 < e0[i] < total for i in gaps)
        flagged[r] = flg
        n_chunks = (n_ops + CHUNK - 1) // CHUNK
        chunk_off.append(chunk_off[-1] + n_chunks)
        for k in range(n_chunks):
            i = CHUNK * k
            table.append((e0[i], t0[i], q0[i], ((ctx[i][0] | (ctx[i][1] << 2)) << 4) | (1 if flg and k == 0 else 0)))
        has_ev = [any(adv[i][0] > 0 for i in range(CHUNK * k, min(CHUNK * k + CHUNK, n_ops))) for k in range(n_chunks)]
        for k in range(n_chunks - 1):      # what K0 carries over a chunk's upper edge
            own = [i for i in range(CHUNK * k, CHUNK * k + CHUNK) if adv[i][0] > 0]
            if not own:
                if any(has_ev[:k]) and any(has_ev[k + 1:]):
                    forks["k0:empty_chunk_between"] += 1
            elif adv[own[-1]][0] >= 2:
                forks["k0:last_long"] += 1
            elif len(own) >= 2:
                forks["k0:last_single_below"] += 1
            else:
                forks["k0:last_single_alone:" + "MIDNSHPMM"[ops[own[0]][1]]] += 1
        # ---- records of the batch ----
        if pos == L - 1: forks["end:pos=L-1"] += 1
        if pos == L: forks["end:pos=L"] += 1
        if pos > L: forks["end:pos>L"] += 1
        if n_ops == 0:
            forks["end:no_ops"] += 1
            with_ops = lambda a, b: any(flat.rec_cig_off[q + 1] > flat.rec_cig_off[q] for q in range(a, b))
            if with_ops(int(flat.contig_rec_off[c]), r) and with_ops(r + 1, int(flat.contig_rec_off[c + 1])):
                forks["end:no_ops_between"] += 1
        if n_ops and all(o in (S, H) for _, o in ops):
            forks["end:clips_only"] += 1
        if t0[-1] > rlen:
            assert q0[-1] > L      # tolerated beyond the contig end only
            forks[f"overhang:{s}"] += 1
        for i, (n, o) in enumerate(ops):
            if o == I and n > 0 and q0[i] in (L - 1, L):
                forks[f"ins:{'L-1' if q0[i] == L - 1 else 'L'}:{s}"] += 1
            if o in (N, P) and 0 < e0[i] < total and not flg:
                forks["noflag:NP_between_events"] += 1
        for i in gaps:
            n, o = ops[i]
            nm = "SH"[o - S] if o in (S, H) else "?"
            if flg and 0 < e0[i] < total:
                k = i // CHUNK
                lo, hi = CHUNK * k, min(CHUNK * k + CHUNK, n_ops)
                if e0[i] > e0[lo] and e0[hi] > e0[i + 1]: forks[f"flag:{nm}:same_chunk"] += 1
                elif e0[hi] == e0[lo]: forks[f"flag:{nm}:eventless_chunk"] += 1
                else: forks[f"flag:{nm}:other_chunk"] += 1
                if n > CHUNK: forks["flag:clip>64"] += 1
            if not flg and e0[i] == total and total > 0 and i + 1 < n_ops and ops[i + 1][1] == P:
                forks["noflag:trailing_clip_then_P"] += 1
            if not flg and e0[i] == 0 and i + 1 < n_ops and sum(adv[i + 1]) == 0 and total > 0:
                forks["noflag:leading_clip_then_zero_ops"] += 1
            if not flg and e0[i] == 0 and n > CHUNK and total > 0:
                forks["noflag:leading_clip>64"] += 1
        col = [i for i in range(n_ops) if adv[i][0] > 0 and ops[i][1] in _KIND]
        on = 0
        for i in range(n_ops):      # events on the contig, op by op
            ev = adv[i][0]
            if ops[i][1] == I: on += ev if q0[i] < L else 0
            elif ev: on += max(0, min(ev, L - q0[i]))
        n_on[r] = on
        if flg:
            if n_ops > 2 * TASK_OPS:
                forks["flag:ops>256"] += 1
                forks["flag:task_k2"] += 1 if n_chunks > 2 else 0
                forks["flag:task_k4"] += 1 if n_chunks > 4 else 0
            continue      # left to k_pileup_flagged_records: no task, no piece
        if not flg and n_ops > 2 * TASK_OPS:
            forks["noflag:ops>256"] += 1
        # ---- strand-specific loads ----
        mcol = [i for i in col if ops[i][1] in _MLIKE and q0[i] < L]
        if s == "f" and col and ops[col[0]][1] in _MLIKE and t0[col[0]] < 4:
            forks[f"fwd_t0:{t0[col[0]]}"] += 1
        if s == "r" and mcol:
            if 1 <= rlen <= 15: forks[f"rev_rlen:{rlen}"] += 1
            left = rlen - (t0[mcol[-1]] + adv[mcol[-1]][0])
            if 0 <= left <= 15: forks[f"rev_end:{left}"] += 1
        # ---- the run form: tasks of NCH chunks ----
        pieces_on = sum(adv[i][0] if q0[i] < L else 0 for i in range(n_ops) if ops[i][1] == I)
        task_np = []
        for j0 in range(0, n_ops, TASK_OPS):
            j1 = min(j0 + TASK_OPS, n_ops)
            tcol = [i for i in col if j0 <= i < j1]
            ps, NP = {}, 0
            for i in tcol:
                ps[i] = NP; NP += (adv[i][0] + PIECE - 1) // PIECE
            task_np.append(NP)
            for v in (0, 255, 256, 257, 512, 513):
                if NP == v: forks[f"np:{v}:{s}"] += 1
            if NP > 0 and NP % 64 == 0: forks[f"np:64k:{s}"] += 1
            if NP > 1 and NP % 64 == 1: forks[f"np:64k+1:{s}"] += 1
            forks[f"windows:{min((NP + MAPW - 1) // MAPW, 3)}{'+' if NP > 2 * MAPW else ''}:{s}"] += 1
            if tcol and q0[j0] >= L: forks[f"task_beyond_contig:{s}"] += 1
            for idx, i in enumerate(tcol):
                (n, o), kind = ops[i], _KIND[ops[i][1]]
                npc = (n + PIECE - 1) // PIECE
                if ps[i] == MAPW - 1 and npc >= 2: forks[f"op_at:255_crossing:{s}"] += 1
                if ps[i] == MAPW: forks[f"op_at:256:{s}"] += 1
                if npc > 2 * MAPW and idx > 0: forks[f"op_gt_512:{kind}:{s}"] += 1
                if any(ps[i] < w0 and ps[i] + npc >= w0 + MAPW for w0 in range(MAPW, NP, MAPW)): forks[f"op_covers_window:{kind}:{s}"] += 1
                # where K1 finds the two events before the op: its own chunk, the lower chunk of the task, K0's entry
                below = [a for a in range(j0, i) if adv[a][0] > 0][::-1]
                where = lambda a: "own" if a // CHUNK == i // CHUNK else "lower"
                if not below: src = "none_first_op" if i == j0 else "none_zero_ops"
                elif adv[below[0]][0] >= 2: src = where(below[0]) + "_" + where(below[0])
                elif len(below) >= 2: src = where(below[0]) + "_" + where(below[1])
                else: src = "one_k0"
                if q0[i] < L:
                    forks[f"lookup:{src}"] += 1
                    at = EDGES.get(i, "in" if i % CHUNK else None)
                    if at:
                        forks[f"ctx:{at}:{_ctx_name(ctx[i], kind)}:{s}"] += 1
                        if at == "in" and i > 0 and sum(adv[i - 1]) == 0:
                            forks[f"ctxz:{_ctx_name(ctx[i], kind)}:{s}"] += 1
                # ---- its pieces ----
                for p in range(npc):
                    off = PIECE * p
                    n_op = min(PIECE, n - off)
                    room = L - (q0[i] + off)
                    if room >= n_op:
                        pieces_on += n_op
                        forks[f"whole:{kind}:{s}" if n_op == PIECE else f"tail:{kind}:{n_op}:{s}"] += 1
                    elif room > 0 or (room == 0 and off > 0):
                        pieces_on += room
                        forks[f"cut:{kind}:{room}:{s}"] += 1
                    else:
                        forks[f"beyond:{kind}:{s}"] += 1
                    if kind == "D" and p >= 1 and room > 0:
                        forks[f"dpiece:{'2' if p == 1 else '3+'}:{s}"] += 1
        for a, b in zip(task_np, task_np[1:]):
            if a == 0 and b > 0: forks[f"np0_then_pieces:{s}"] += 1
        assert pieces_on == on, (r, pieces_on, on)      # the pieces and the ops count the same events
    tab = np.array(table, np.int64).reshape(-1, 4).astype(np.int32)
    return types.SimpleNamespace(forks=forks, chunk_table=tab, chunk_off=np.array(chunk_off, np.int64), flagged=flagged, n_events=n_events, n_on_contig=n_on)


# ------------------------------------------------------------------------------------------------
# what every case must reach
# ------------------------------------------------------------------------------------------------
def _fr(names):
    return [f"{n}:{s}" for n in names for s in "fr"]


ALL_CTX = [_ctx_name(c, k) for c in CONTEXTS for k in "MD"]
assert len(ALL_CTX) == 14
FORKS = {
    "context": _fr([f"ctx:in:{c}" for c in ALL_CTX] + [f"ctxz:{c}" for c in ALL_CTX]),
    "boundaries": _fr([f"ctx:{e}:{c}" for e in EDGES.values() for c in ALL_CTX])
    + ["k0:last_long", "k0:last_single_below", "k0:last_single_alone:D", "k0:last_single_alone:I", "k0:empty_chunk_between", "lookup:own_own", "lookup:own_lower",
       "lookup:lower_lower", "lookup:one_k0", "lookup:none_first_op", "lookup:none_zero_ops"],
    "pieces": _fr([f"tail:{k}:{n}" for k in "MD" for n in range(1, 16)] + [f"cut:{k}:{n}" for k in "MD" for n in range(16)] + ["dpiece:2", "dpiece:3+", "whole:M", "whole:D",
                  "beyond:M", "beyond:D", "ins:L-1", "ins:L", "overhang"])
    + [f"fwd_t0:{t}" for t in range(4)] + [f"rev_rlen:{n}" for n in range(1, 16)] + [f"rev_end:{n}" for n in range(16)],
    "windows": _fr(["np:0", "np:255", "np:256", "np:257", "np:512", "np:513", "np:64k", "np:64k+1", "op_at:255_crossing", "op_at:256", "op_gt_512:M", "op_gt_512:D",
                    "op_covers_window:M", "op_covers_window:D", "np0_then_pieces", "task_beyond_contig", "windows:1", "windows:2", "windows:3+"]),
    "flags": ["flag:S:same_chunk", "flag:H:same_chunk", "flag:S:eventless_chunk", "flag:H:eventless_chunk", "flag:S:other_chunk", "flag:H:other_chunk",
              "noflag:trailing_clip_then_P", "noflag:leading_clip_then_zero_ops", "noflag:NP_between_events", "flag:ops>256", "flag:task_k2", "flag:task_k4",
              "flag:clip>64", "noflag:leading_clip>64", "noflag:ops>256"],
    "ends": ["end:pos=L-1", "end:pos=L", "end:pos>L", "end:no_ops_between", "end:clips_only", "end:L=1", "end:L=2", "end:L=3", "end:L=17",
             "end:contig_without_records_between"],
}
