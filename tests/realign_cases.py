"""The cut and the join of the CIGAR-less route (k_realign_cut, k_anchor_join_plan, k_anchor_join; hairsplitter_amd/csrc/hs_kernels_realign.hip) restated in
numpy, the cases that reach each of their forks, and the jobs whose piece classes sit on the section seams of realign_job (hs_capi_realign.inc).

cut(seq, off, src, rev) is the whole output buffer of k_realign_cut, join_plan(table) what k_anchor_join_plan leaves and join(table, plan) the whole joined
buffer, zeros behind the moves and behind the last interval included. A cut case is a dict seq / off / src / rev (rev may be None) with `reach`: the
forks it claims; cut_forks(case) computes from the layout alone which forks a case reaches, and tests/test_cpu_realign_cases.py holds the two against each
other. A join case is a piece table as realign_job builds it with the aligner's side made up: join_table() derives dist, start, end and len from every
piece's move string. tests/test_gpu_realign_cases.py runs the cases through api.realign_cut_tap / api.anchor_join_tap and compares whole buffers."""
import functools

import numpy as np

import anchor_cases as ac

HW, HEAD, MID, TAIL, INS = range(5)
KIND_NAME = ("HW", "HEAD", "MID", "TAIL", "INS")


def _rng(*seed):
    return np.random.default_rng([0x5243] + list(seed))


def round16(n):
    return (int(n) + 15) & ~15


# ------------------------------------------------------------------------------------------------
# the cut
# ------------------------------------------------------------------------------------------------
def cut(seq, off, src, rev):
    """out[off[i] + k] = seq[src[i] + k], or (3 - seq[src[i] - k]) mod 256 where rev[i] is set; zeros from off[m] to the next multiple of 16"""
    seq, off, src = np.asarray(seq, np.uint8), np.asarray(off, np.int64), np.asarray(src, np.int64)
    n = np.diff(off)
    r = np.zeros(len(src), bool) if rev is None else np.asarray(rev) != 0
    k = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], n)
    rr = np.repeat(r, n)
    b = seq[np.repeat(src, n) + np.where(rr, -k, k)]
    out = np.zeros(round16(off[-1]), np.uint8)
    out[:off[-1]] = np.where(rr, (3 - b.astype(np.int64)) & 0xff, b).astype(np.uint8)
    return out


def cut_case(seq, pieces, rev_null=False, reach=()):
    """pieces: [(length, src, rev)] in output order"""
    off = np.concatenate([[0], np.cumsum([p[0] for p in pieces])]).astype(np.int64)
    assert not rev_null or not any(p[2] for p in pieces)
    return dict(seq=np.asarray(seq, np.uint8), off=off, src=np.array([p[1] for p in pieces], np.int64), rev=None if rev_null else np.array([p[2] for p in pieces], np.uint8),
                reach=tuple(reach))


def cut_pieces(case):
    rev = np.zeros(len(case["src"]), np.uint8) if case["rev"] is None else case["rev"]
    return [(int(n), int(s), int(r)) for n, s, r in zip(np.diff(case["off"]), case["src"], rev)]


def cut_reordered(case, order):
    """the same pieces in another output order"""
    p = cut_pieces(case)
    return cut_case(case["seq"], [p[i] for i in order], rev_null=case["rev"] is None, reach=())


def cut_refusal(seq_len, off, src, rev, m=None, out_cap=None):
    """the message hs_realign_cut_tap refuses the tables with (its beginning), or None: the predicates of its host checks"""
    m = len(src) if m is None else m
    if seq_len < 1 or m < 1:
        return "hs_realign_cut_tap: bad arguments"
    if off[0] != 0:
        return "hs_realign_cut_tap: off must ascend strictly from 0"
    for i in range(m):
        n = int(off[i + 1]) - int(off[i])
        if n < 1:
            return "hs_realign_cut_tap: off must ascend strictly from 0"
        r = rev is not None and rev[i]
        lo, hi = (src[i] - (n - 1), src[i]) if r else (src[i], src[i] + n - 1)
        if lo < 0 or hi >= seq_len:
            return "hs_realign_cut_tap: piece %d " % i
    if out_cap is not None and out_cap < round16(off[m]):
        return "hs_realign_cut_tap: out_cap %d is below" % out_cap
    return None


def cut_forks(case):
    """which forks of k_realign_cut the layout reaches: per 16-byte block the whole-block path (forward / reversed, at each source residue mod 4, ending
    exactly on its piece's end) or the byte path (one byte short of whole, over a forward | reversed boundary, over >= 3 or 16 pieces, with bytes behind
    off[m]); per 4096-byte window p_lo == p_hi or more than 256 pieces; what off[m] is a multiple of; where the pieces begin and what their sources touch"""
    off, src, seq_len = case["off"], case["src"], len(case["seq"])
    m, total = len(src), int(off[-1])
    rev = np.zeros(m, np.uint8) if case["rev"] is None else case["rev"]
    f = set()
    f.add("rev NULL" if case["rev"] is None else "rev given")
    f.add("m == 1" if m == 1 else "m > 1")
    f.add("off[m] % 4096 == 0" if total % 4096 == 0 else ("off[m] % 16 == 0" if total % 16 == 0 else "off[m] % 16 != 0"))
    piece_of = lambda a: int(np.searchsorted(off, a, side="right")) - 1
    for a in range(0, round16(total), 16):
        i = piece_of(a)
        if a + 16 <= off[i + 1]:
            k = a - int(off[i])
            p = int(src[i]) - k - 15 if rev[i] else int(src[i]) + k
            f.add("block %s sh %d" % ("rev" if rev[i] else "fwd", p % 4))
            if a + 16 == off[i + 1]:
                f.add("block a + 16 == off[i + 1]")
            if rev[i] and p < 4:
                f.add("block rev loads seq[0]")
            if not rev[i] and p + 16 > seq_len - 4:
                f.add("block fwd loads seq[seq_len - 1]")
        else:
            j = piece_of(min(a + 15, total - 1))
            f.add("bytes")
            if a + 16 == off[i + 1] + 1:
                f.add("bytes a + 16 == off[i + 1] + 1")
            if any(rev[x] != rev[x + 1] for x in range(i, j)):
                f.add("bytes fwd | rev")
            if j - i + 1 >= 3:
                f.add("bytes >= 3 pieces")
            if j - i + 1 == 16:
                f.add("bytes 16 pieces")
            if a + 16 > total:
                f.add("bytes behind off[m]")
    for win in range(0, round16(total), 4096):
        lo, hi = piece_of(win), piece_of(min(win + 4095, total - 1))
        if lo == hi:
            f.add("window p_lo == p_hi")
        if hi - lo + 1 > 256:
            f.add("window > 256 pieces")
    for i in range(m):
        n = int(off[i + 1] - off[i])
        f.add("piece begins at %d mod 16" % (off[i] % 16))
        f.add("src %s %d mod 4" % ("rev" if rev[i] else "fwd", src[i] % 4))
        f.add("length %d" % n)
        if rev[i] and src[i] - (n - 1) == 0:
            f.add("rev piece ends on seq[0]")
        if not rev[i] and src[i] + n == seq_len:
            f.add("fwd piece ends on seq[seq_len - 1]")
    return f


def cut_refused():
    """[(name, arguments of api.realign_cut_tap, seq_len, the message's beginning)]: one table per host check of hs_realign_cut_tap, each a step outside"""
    seq = np.arange(100, dtype=np.uint8) & 3
    good = dict(seq=seq, off=[0, 10, 30], src=[5, 60], rev=[0, 1])
    out = []
    def bad(name, msg, **kw):
        a = dict(good, **kw)
        out.append((name, a, len(a["seq"]), msg))
    bad("no_pieces", "hs_realign_cut_tap: bad arguments", off=[0], src=[], rev=[], m=0)
    bad("off_begins_at_1", "hs_realign_cut_tap: off must ascend strictly from 0", off=[1, 10, 30])
    bad("off_stays", "hs_realign_cut_tap: off must ascend strictly from 0", off=[0, 10, 10])
    bad("off_falls", "hs_realign_cut_tap: off must ascend strictly from 0", off=[0, 10, 9])
    bad("forward_src_negative", "hs_realign_cut_tap: piece 0 ", src=[-1, 60])
    bad("forward_past_the_end", "hs_realign_cut_tap: piece 0 ", src=[91, 60])
    bad("reversed_before_the_start", "hs_realign_cut_tap: piece 1 ", src=[5, 18])
    bad("reversed_src_at_seq_len", "hs_realign_cut_tap: piece 1 ", src=[5, 100])
    bad("short_out_cap", "hs_realign_cut_tap: out_cap 31 is below", out_cap=31)
    return good, out


CUT_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097)


def _cut_cases():
    g = _rng(1)
    S = 20000
    seq = g.integers(0, 4, size=S).astype(np.uint8)
    place = lambda n, r: int(g.integers(n, S - n)) if r else int(g.integers(0, S - n))
    c = {}
    # every length the issue names, forward then reversed: a piece of 4096 and its neighbours put every later boundary at another residue
    c["lengths"] = cut_case(seq, [(n, place(n, r), r) for r in (0, 1) for n in CUT_LENGTHS], reach=["length %d" % n for n in CUT_LENGTHS] + ["block fwd sh 0", "block rev sh 0", "bytes"])
    # a whole window inside one piece, on either strand
    c["window_inside_a_piece"] = cut_case(seq, [(100, 50, 0), (8300, 300, 0), (8300, 9000, 1)], reach=["window p_lo == p_hi", "block fwd sh 0", "block rev sh 1"])
    # pieces of 33 on alternating strands: they begin at 0, 33, 66, ...: every residue mod 16, and each holds a whole block
    c["every_output_residue"] = cut_case(seq, [(33, place(33, i & 1), i & 1) for i in range(17)], reach=["piece begins at %d mod 16" % r for r in range(16)] + ["bytes fwd | rev"])
    # pieces of 48 from an aligned output offset: whole blocks only, their sources at every residue mod 4 on either strand
    c["every_source_residue"] = cut_case(seq, [(48, 1000 + 100 * (2 * s + r) + s, r) for s in range(4) for r in (0, 1)],
                                         reach=["src %s %d mod 4" % (d, s) for d in ("fwd", "rev") for s in range(4)] + ["block %s sh %d" % (d, s) for d in ("fwd", "rev") for s in range(4)]
                                         + ["off[m] % 16 == 0"])
    # a block that ends exactly on its piece's end, and the next one a byte short of whole
    c["block_ends_on_the_piece"] = cut_case(seq, [(16, 700, 1), (15, 900, 0), (17, 1100, 1), (32, 1300, 0), (15, 1500, 1), (6, 1700, 0)],
                                            reach=["block a + 16 == off[i + 1]", "bytes a + 16 == off[i + 1] + 1", "off[m] % 16 != 0", "bytes behind off[m]"])
    # 300 pieces of one base, strands alternating: blocks of 16 pieces, a window of more than 256
    c["one_base_pieces"] = cut_case(seq, [(1, int(x), i & 1) for i, x in enumerate(g.integers(0, S, size=300))], reach=["bytes 16 pieces", "window > 256 pieces", "bytes fwd | rev", "bytes >= 3 pieces"])
    c["forward_reversed_boundary"] = cut_case(seq, [(24, 500, 0), (24, 800, 1)], reach=["bytes fwd | rev", "off[m] % 16 == 0"])
    c["one_piece_of_a_window"] = cut_case(seq, [(4096, 2000, 0)], rev_null=True, reach=["m == 1", "rev NULL", "off[m] % 4096 == 0", "window p_lo == p_hi"])
    c["rev_null_many"] = cut_case(seq, [(n, place(n, 0), 0) for n in (5, 4, 3, 100, 16)], rev_null=True, reach=["rev NULL", "m > 1", "bytes >= 3 pieces"])
    # reversed pieces whose last base is seq[0]: the block that holds it loads from the address of seq[0] - sh on; forward fillers keep the offsets aligned
    small = g.integers(0, 4, size=40).astype(np.uint8)
    c["reversed_ends_on_seq_0"] = cut_case(small, [x for r in range(4) for x in ((32 + r, 31 + r, 1), (16 - r, 5, 0))],
                                           reach=["rev piece ends on seq[0]", "block rev loads seq[0]"] + ["block rev sh %d" % r for r in range(4)])
    # forward pieces whose last base is the sequence's last: the block's fifth dword lies behind it, in the pad
    for L in (40, 41, 42, 43):
        tail = g.integers(0, 4, size=L).astype(np.uint8)
        c["forward_ends_on_the_last_base_%d" % L] = cut_case(tail, [(32, L - 32, 0), (L - 3, 3, 0)], reach=["fwd piece ends on seq[seq_len - 1]", "block fwd loads seq[seq_len - 1]"])
    # every byte value, reversed: by whole blocks (complement4), and with a boundary in every block (3 - b)
    allb = np.concatenate([g.integers(0, 4, size=64).astype(np.uint8), np.arange(256, dtype=np.uint8), g.integers(0, 4, size=64).astype(np.uint8)])
    c["all_bytes_by_blocks"] = cut_case(allb, [(256, 64 + 255, 1), (256, 64, 0)], reach=["block rev sh 0", "block fwd sh 0"])
    c["all_bytes_by_bytes"] = cut_case(allb, [(4, 10, 0)] + [(8, 64 + 8 * j + 7, 1) for j in range(32)] + [(4, 20, 1)], reach=["bytes", "off[m] % 16 != 0"])
    return c


CUT_CASES = _cut_cases()


def cut_block_paths(case):
    """per 16-byte block of the output: True where k_realign_cut takes the whole-block path"""
    off, total = case["off"], int(case["off"][-1])
    a = np.arange(0, round16(total), 16)
    i = np.searchsorted(off, a, side="right") - 1
    return a + 16 <= off[i + 1]


# ------------------------------------------------------------------------------------------------
# the join
# ------------------------------------------------------------------------------------------------
def piece_numbers(kind, moves, start=0):
    """(dist, start, end, len) of a piece as the aligner leaves them for its move string (a head's: of the two reversed strings): one edit per move that is
    not '=', the target bases from `start` on (HW only; 0 for the other modes) to `end`, which the non-I moves consume: end - start + 1 of them"""
    mv = np.asarray(moves, np.uint8)
    start = start if kind == HW else 0
    end = start + int((mv != 1).sum()) - 1
    assert end - start + 1 == int((mv != 1).sum())
    return int((mv != 0).sum()), start, end, len(mv)


def join_table(intervals, slack=None, seed=0, ops_residue=None, order=None):
    """intervals: [dict(base, pieces=[(kind, moves | INS count, optional dict of overrides: len, start, extra (target bases beyond those consumed))], room_extra)].
    The pieces get their numbers at shuffled indices and their moves at shuffled places in `ops` (order: of the intervals in the table; ops_residue: the
    residue mod 4 every piece's moves begin at). Returns the table api.anchor_join_tap takes, with `moves` (per piece, as given) for the restatements."""
    g = _rng(2, seed)
    order = list(range(len(intervals))) if order is None else list(order)
    iv_piece, iv_base, join_off = [0], [], [0]
    kind, idx, room, given, over = [], [], [], [], []
    for k in order:
        iv = intervals[k]
        rooms = 0
        for pc in iv["pieces"]:
            kd, mv = pc[0], pc[1]
            o = dict(pc[2]) if len(pc) > 2 else {}
            if kd == INS:
                kind.append(INS); idx.append(int(mv)); room.append(int(o.get("room", mv))); given.append(None)
            else:
                mv = np.asarray(mv, np.uint8)
                kind.append(kd); idx.append(-1); given.append(mv)
                room.append(int((mv != 2).sum()) + int((mv != 1).sum()) + int(o.get("extra", 0)))      # query bases + target bases
                assert room[-1] >= len(mv)
            over.append(o)
            rooms += room[-1]
        iv_piece.append(len(kind)); iv_base.append(int(iv["base"]))
        join_off.append(join_off[-1] + rooms + int(iv.get("room_extra", 0)))
    P = len(kind)
    real = [p for p in range(P) if kind[p] != INS]
    n_num = len(real) + 3
    slots = g.permutation(n_num)[:len(real)]
    num = {f: g.integers(-50, 50, size=n_num).astype(np.int32) for f in ("dist", "start", "end", "len")}      # (the unused numbers are junk)
    pc_ops = np.zeros(P, np.int64)
    at = int(g.integers(0, 8))
    chunks = []
    for p in g.permutation(len(real)):
        p = real[p]
        if ops_residue is not None:
            at += (ops_residue - at) % 4
        else:
            at += int(g.integers(0, 4))
        pc_ops[p] = at
        chunks.append((at, given[p]))
        at += room[p]
    ops = g.integers(0, 4, size=at + 8).astype(np.uint8)      # (junk between and behind the moves)
    for a, mv in chunks:
        ops[a:a + len(mv)] = mv
    for p, s in zip(real, slots):
        idx[p] = int(s)
        d, st, en, ln = piece_numbers(kind[p], given[p], start=int(over[p].get("start", 0)))
        ln = over[p].get("len", ln)      # (a piece the aligner has no path for: -1, 0, or more moves than its room)
        num["dist"][s], num["start"][s], num["end"][s], num["len"][s] = d, st, en, room[p] + 1 if ln == "room + 1" else ln
    return dict(iv_piece=np.array(iv_piece, np.int32), iv_base=np.array(iv_base, np.int32), join_off=np.array(join_off, np.int64), pc_kind=np.array(kind, np.uint8),
                pc_idx=np.array(idx, np.int32), pc_room=np.array(room, np.int32), pc_ops=pc_ops, ops=ops, moves=given, order=order, **num)


def join_plan(t):
    """k_anchor_join_plan: pc_at, out_len, out_dist, out_pos"""
    m, P = len(t["iv_base"]), len(t["pc_kind"])
    kind, idx = t["pc_kind"].astype(np.int64), t["pc_idx"].astype(np.int64)
    ins = kind == INS
    safe = np.where(ins, 0, idx)
    n = np.where(ins, idx, t["len"].astype(np.int64)[safe] if len(t["len"]) else 0)
    d = np.where(ins, idx, t["dist"].astype(np.int64)[safe])
    shift = np.where(kind == HW, t["start"].astype(np.int64)[safe], 0) - np.where(kind == HEAD, t["end"].astype(np.int64)[safe] + 1, 0)
    ok_piece = (n > 0) & (n <= t["pc_room"])
    grow = np.maximum(n, 0)
    before = np.concatenate([[0], np.cumsum(grow)])
    p0, p1 = t["iv_piece"][:-1].astype(np.int64), t["iv_piece"][1:].astype(np.int64)
    of = np.repeat(np.arange(m), p1 - p0)
    pc_at = before[:-1] - before[p0][of]
    total = before[p1] - before[p0]
    ok = np.logical_and.reduceat(ok_piece, p0) & (total <= np.diff(t["join_off"]))
    dist, pos = np.add.reduceat(d, p0), t["iv_base"].astype(np.int64) + np.add.reduceat(shift, p0)
    i32 = lambda a: a.astype(np.int64).astype(np.int32)
    return dict(pc_at=i32(pc_at), out_len=i32(np.where(ok, total, -1)), out_dist=i32(np.where(ok, dist, -1)), out_pos=i32(np.where(ok, pos, -1)))


def join(t, plan):
    """k_anchor_join: the joined buffer, join_off[m] rounded up to 16 bytes: a kept interval's pieces back to back (a head's moves turned, an INS run as 1s),
    zeros everywhere else"""
    out = np.zeros(round16(t["join_off"][-1]), np.uint8)
    for k in np.flatnonzero(plan["out_len"] > 0):
        for p in range(int(t["iv_piece"][k]), int(t["iv_piece"][k + 1])):
            a = int(t["join_off"][k]) + int(plan["pc_at"][p])
            if t["pc_kind"][p] == INS:
                out[a:a + int(t["pc_idx"][p])] = 1
            else:
                n = int(t["len"][t["pc_idx"][p]])
                mv = t["ops"][int(t["pc_ops"][p]):int(t["pc_ops"][p]) + n]
                out[a:a + n] = mv[::-1] if t["pc_kind"][p] == HEAD else mv
    return out


def join_stitched(t):
    """(pos, NM, moves) of every interval by anchor_cases.stitch: the head is placed by its count of non-I moves, not by end + 1. None where a piece has no path"""
    out = []
    for k in range(len(t["iv_base"])):
        pcs, aligned, ok = [], [], True
        base = int(t["iv_base"][k])
        for p in range(int(t["iv_piece"][k]), int(t["iv_piece"][k + 1])):
            kd = int(t["pc_kind"][p])
            if kd == INS:
                n = int(t["pc_idx"][p])
                ok = ok and 0 < n <= t["pc_room"][p]
                pcs.append(("INS", 0, n, base, base)); aligned.append(None)
                continue
            i = int(t["pc_idx"][p])
            n = int(t["len"][i])
            ok = ok and 0 < n <= t["pc_room"][p]
            mv = t["moves"][p]
            ok = ok and n == len(mv)
            # (t0, t1): a first HW piece begins at the window's start, a first MID at the first anchor; a head ends on it
            pcs.append((KIND_NAME[kd], 0, int((mv != 2).sum()), base, base)); aligned.append((int(t["dist"][i]), int(t["start"][i]), int(t["end"][i]), mv))
        out.append(ac.stitch(pcs, aligned) if ok else None)
    return out


def join_refusal(t, joined_cap=None):
    """the message hs_anchor_join_tap refuses the table with (its beginning), or None: the predicates of its host checks"""
    who = "hs_anchor_join_tap: "
    m, n_num, nb = len(t["iv_base"]), len(t["dist"]), len(t["ops"])
    if m < 1:
        return who + "bad arguments"
    if t["iv_piece"][0] != 0 or t["join_off"][0] != 0:
        return who + "iv_piece and join_off must ascend from 0"
    for k in range(m):
        if t["iv_piece"][k + 1] <= t["iv_piece"][k]:
            return who + "interval %d has no pieces" % k
        if t["join_off"][k + 1] < t["join_off"][k]:
            return who + "join_off must ascend from 0 (interval %d)" % k
    for k in range(m):
        rooms = 0
        for p in range(int(t["iv_piece"][k]), int(t["iv_piece"][k + 1])):
            if t["pc_kind"][p] > INS:
                return who + "piece %d is of kind" % p
            if t["pc_room"][p] < 0:
                return who + "piece %d has a negative room" % p
            if t["pc_kind"][p] != INS:
                if not 0 <= t["pc_idx"][p] < n_num:
                    return who + "piece %d names the numbers at" % p
                if t["pc_ops"][p] < 0 or t["pc_ops"][p] + t["pc_room"][p] > nb:
                    return who + "piece %d has its moves at" % p
            rooms += int(t["pc_room"][p])
        room = int(t["join_off"][k + 1] - t["join_off"][k])
        if room < rooms or room > 0x7fffffff:
            return who + "interval %d has room for" % k
    if joined_cap is not None and joined_cap < round16(t["join_off"][-1]):
        return who + "joined_cap %d is below" % joined_cap
    return None


def join_refused():
    """(a good table, [(name, the table a step outside one host check of hs_anchor_join_tap, joined_cap or None, the message's beginning)])"""
    good = join_case("blocks_over_pieces")
    who = "hs_anchor_join_tap: "
    out = []
    def bad(name, msg, joined_cap=None, **kw):
        t = dict(good)
        for k, (i, v) in kw.items():
            a = np.array(t[k])
            a[i] = v
            t[k] = a
        out.append((name, t, joined_cap, who + msg))
    P, n_num, nb = len(good["pc_kind"]), len(good["dist"]), len(good["ops"])
    first_real = int(np.flatnonzero(good["pc_kind"] != INS)[0])
    last_ops = int(np.argmax(good["pc_ops"] + good["pc_room"]))
    bad("iv_piece_begins_at_1", "iv_piece and join_off must ascend from 0", iv_piece=(0, 1))
    bad("join_off_begins_at_1", "iv_piece and join_off must ascend from 0", join_off=(0, 1))
    bad("interval_without_pieces", "interval 0 has no pieces", iv_piece=(1, 0))
    bad("iv_piece_falls", "interval 1 has no pieces", iv_piece=(2, int(good["iv_piece"][1]) - 1))
    bad("join_off_falls", "join_off must ascend from 0 (interval 1)", join_off=(2, int(good["join_off"][1]) - 1))
    bad("kind_5", "piece 1 is of kind", pc_kind=(1, 5))
    bad("negative_room", "piece 1 has a negative room", pc_room=(1, -1))
    bad("numbers_below", "piece %d names the numbers at" % first_real, pc_idx=(first_real, -1))
    bad("numbers_above", "piece %d names the numbers at" % first_real, pc_idx=(first_real, n_num))
    bad("moves_below", "piece %d has its moves at" % first_real, pc_ops=(first_real, -1))
    bad("moves_above", "piece %d has its moves at" % last_ops, pc_ops=(last_ops, nb - int(good["pc_room"][last_ops]) + 1))
    bad("room_below_the_pieces", "interval 0 has room for", pc_room=(0, int(good["pc_room"][0]) + int(good["join_off"][1]) - int(good["pc_room"][:good["iv_piece"][1]].sum()) + 1))
    bad("short_joined_cap", "joined_cap %d is below" % (round16(good["join_off"][-1]) - 1), joined_cap=round16(good["join_off"][-1]) - 1)
    return good, out


def join_forks(t, plan):
    """which forks of k_anchor_join the table reaches: per 16-byte block the whole-block path by kind (a head's at each address residue of its load) or the
    byte path (over 2, >= 3 or 16 pieces, over two intervals, over the slack behind an interval's moves, inside a dropped interval, behind join_off[m]); a
    4096-byte seam inside a piece or on an interval boundary; what join_off[m] is a multiple of; the plan's grid; the first piece's kind per interval"""
    f = set()
    jo, m = t["join_off"].astype(np.int64), len(t["iv_base"])
    total = int(jo[-1])
    f.add("join_off[m] % 16 == 0" if total % 16 == 0 else "join_off[m] % 16 != 0")
    f.add("m == %d" % m if m in (1, 256, 257) else "m other")
    # per byte of the buffer: its interval and its piece (-1: no move there)
    iv = np.searchsorted(jo, np.arange(round16(total)), side="right") - 1
    piece = np.full(round16(total), -1, np.int64)
    for k in range(m):
        p0, p1 = int(t["iv_piece"][k]), int(t["iv_piece"][k + 1])
        f.add("first piece %s" % KIND_NAME[t["pc_kind"][p0]])
        if plan["out_len"][k] <= 0:
            f.add("dropped interval %s" % ("first" if k == 0 else ("last" if k == m - 1 else "middle")))
            continue
        ends = np.concatenate([plan["pc_at"][p0 + 1:p1], [plan["out_len"][k]]])
        for p, e in zip(range(p0, p1), ends):
            piece[jo[k] + plan["pc_at"][p]:jo[k] + e] = p
            f.add("%s of %d moves" % (KIND_NAME[t["pc_kind"][p]], e - plan["pc_at"][p]))
    iv[total:] = m
    for a in range(0, round16(total), 16):
        ps, ks = piece[a:a + 16], iv[a:a + 16]
        if (ps == ps[0]).all() and ps[0] >= 0:
            p = int(ps[0])
            kd = int(t["pc_kind"][p])
            f.add("block %s" % KIND_NAME[kd])
            if kd == HEAD:
                k = int(ks[0])
                n = int(t["len"][t["pc_idx"][p]])
                x_in = a - int(jo[k]) - int(plan["pc_at"][p])
                f.add("block HEAD load at %d mod 4" % ((int(t["pc_ops"][p]) + n - 16 - x_in) % 4))
        else:
            f.add("bytes")
            real = [x for x in ps.tolist() if x >= 0]
            n_p = len(set(real))
            if n_p == 2:
                f.add("bytes 2 pieces")
            if n_p >= 3:
                f.add("bytes >= 3 pieces")
            if n_p == 16:
                f.add("bytes 16 pieces")
            kk = [x for x in ks.tolist() if x < m]
            if len(set(kk)) >= 2:
                f.add("bytes 2 intervals")
                cut = int(np.flatnonzero(ks != ks[0])[0])
                if ps[0] >= 0 and (ps[:cut] == -1).any() and ps[cut] >= 0:
                    f.add("bytes 2 intervals with slack")
            if any(plan["out_len"][x] <= 0 for x in set(kk)):
                f.add("bytes in a dropped interval")
            if a + 16 > total:
                f.add("bytes behind join_off[m]")
    for seam in range(4096, total, 4096):
        if piece[seam] >= 0 and piece[seam] == piece[seam - 1]:
            f.add("4096 seam inside a piece")
        if seam in jo.tolist():
            f.add("4096 seam on an interval boundary")
    return f


def _moves(g, n, mix=(0.7, 0.05, 0.05, 0.2)):
    """n moves, '=' and X mixed inside the M runs; never without a non-I move in a piece of more than one move (so that a head consumes a target base)"""
    mv = g.choice(4, size=n, p=mix).astype(np.uint8)
    if n and (mv == 1).all():
        mv[0] = 3
    return mv


JOIN_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 1100)


def _join_cases():
    """name -> (intervals, keyword arguments of join_table, the forks the case claims)"""
    g = _rng(3)
    mv = lambda n: _moves(g, n)
    c = {}
    # every kind at every length; heads first, an HW interval, INS at either end
    ivs = [dict(base=500, pieces=[(HW, mv(1100), dict(start=37, extra=200))])]
    ivs += [dict(base=1000 + 100 * n, pieces=[(HEAD, mv(n), dict(extra=9)), (MID, mv(n)), (TAIL, mv(n), dict(extra=20))], room_extra=n % 5) for n in JOIN_LENGTHS]
    ivs += [dict(base=7, pieces=[(INS, 5), (MID, mv(33)), (INS, 3)]), dict(base=90, pieces=[(MID, mv(16)), (MID, mv(1)), (TAIL, mv(15))]), dict(base=3, pieces=[(HW, mv(1), dict(start=2))])]
    c["kinds_and_lengths"] = (ivs, {}, ["first piece HW", "first piece HEAD", "first piece INS", "first piece MID", "block HW", "block HEAD", "block MID", "block TAIL", "bytes"]
                              + ["%s of %d moves" % (k, n) for k in ("HEAD", "MID", "TAIL") for n in JOIN_LENGTHS])
    # heads of 48 moves in intervals whose rooms are multiples of 16: whole blocks, the moves at each address residue
    for r in range(4):
        ivs = [dict(base=100 * i, pieces=[(HEAD, _moves(g, 48, (0.5, 0.0, 0.0, 0.5))), (MID, _moves(g, 16, (0.5, 0.0, 0.0, 0.5)))], room_extra=0) for i in range(3)]
        c["head_blocks_ops_at_%d_mod_4" % r] = (ivs, dict(ops_residue=r), ["block HEAD load at %d mod 4" % r, "block MID", "join_off[m] % 16 == 0"])
    c["ins_block"] = ([dict(base=10, pieces=[(INS, 40), (MID, mv(8))]), dict(base=20, pieces=[(MID, mv(4)), (INS, 35)], room_extra=3)], {}, ["block INS", "first piece INS", "bytes 2 pieces"])
    # (moves 0 and 3 only: a piece of n moves has room for 2 n, so the intervals begin at multiples of 16)
    m03 = lambda n: _moves(g, n, (0.5, 0.0, 0.0, 0.5))
    c["blocks_over_pieces"] = ([dict(base=3, pieces=[(MID, m03(1)) for _ in range(16)]), dict(base=1, pieces=[(MID, m03(8)), (MID, m03(8))]),
                                dict(base=2, pieces=[(HEAD, m03(5)), (MID, m03(5)), (TAIL, m03(6))])], {}, ["bytes 2 pieces", "bytes >= 3 pieces", "bytes 16 pieces"])
    # (mostly I and D: a piece's room is little above its moves, so a block holds the end of one interval, its slack and the next one's first moves)
    mid = lambda n: _moves(g, n, (0.1, 0.45, 0.45, 0.0))
    c["slack_between_intervals"] = ([dict(base=5 * i, pieces=[(HEAD, mid(9)), (TAIL, mid(11), dict(extra=1))], room_extra=1) for i in range(6)], {},
                                    ["bytes 2 intervals with slack", "bytes 2 intervals", "join_off[m] % 16 != 0", "bytes behind join_off[m]"])
    for bad in (-1, 0, "room + 1"):
        ivs = []
        for i in range(5):
            pcs = [(HEAD, mv(20), dict(extra=2)), (MID, mv(30)), (TAIL, mv(25), dict(extra=6))]
            if i in (0, 2, 4):
                j = i // 2
                pcs[j] = (pcs[j][0], pcs[j][1], dict(pcs[j][2] if len(pcs[j]) > 2 else {}, len=bad))
            ivs.append(dict(base=40 * i + 100, pieces=pcs, room_extra=i))
        c["dropped_len_%s" % str(bad).replace(" ", "_")] = (ivs, {}, ["dropped interval first", "dropped interval middle", "dropped interval last", "bytes in a dropped interval"])
    # a piece over the 4096-byte seam; then rooms that put an interval boundary on the next one
    a = [dict(base=0, pieces=[(MID, mv(1000)), (MID, mv(1000))]), dict(base=9, pieces=[(HEAD, mv(1100), dict(extra=5))])]
    used = sum(2 * len(p[1]) - int((p[1] == 1).sum()) - int((p[1] == 2).sum()) + (p[2]["extra"] if len(p) > 2 else 0) for iv in a for p in iv["pieces"])
    assert 4096 < used < 8192
    a[1]["room_extra"] = 8192 - used
    a.append(dict(base=77, pieces=[(TAIL, mv(40), dict(extra=8))]))
    c["window_seams"] = (a, {}, ["4096 seam inside a piece", "4096 seam on an interval boundary"])
    for m in (1, 256, 257):
        c["plan_grid_m_%d" % m] = ([dict(base=i, pieces=[(MID, _moves(g, 3))]) for i in range(m)], {}, ["m == %d" % m])
    return c


JOIN_CASES = _join_cases()


@functools.lru_cache(maxsize=None)
def join_case(name, shuffled=False):
    """the table of a case; shuffled: the intervals in another order, the moves at other places"""
    ivs, kw, _ = JOIN_CASES[name]
    order = _rng(4, len(ivs)).permutation(len(ivs)) if shuffled else None
    return join_table(ivs, seed=1 if shuffled else 0, order=order, **kw)


# ------------------------------------------------------------------------------------------------
# route jobs: realign_job's class sections (numbers from a multiple of 64, moves from a multiple of 256)
# ------------------------------------------------------------------------------------------------
ROUTE_CASES = {"hw63_shw64_nw65": (63, 64, 65), "hw64_shw65_nw63": (64, 65, 63), "hw65_shw63_nw64": (65, 63, 64), "first_class_empty": (0, 5, 7)}


@functools.lru_cache(maxsize=None)
def route_job(name):
    """a job in the shape of tests/test_gpu_map_anchors.py's: one contig, reads of 120 bases with a few substitutions, n_hw intervals without anchors and
    anchored ones whose heads and tails count n_shw and whose middles count n_nw; anchors on the true diagonal"""
    n_hw, n_shw, n_nw = ROUTE_CASES[name]
    g = _rng(5, n_hw, n_shw, n_nw)
    L = 120
    n_anch = (n_shw + 1) // 2
    assert n_nw >= n_anch - 1
    C = g.integers(0, 4, size=(n_hw + n_anch) * 150 + 400).astype(np.uint8)
    reads, ivs, ancs = [], [], []
    for i in range(n_hw + n_anch):
        start = 200 + 150 * i
        read = C[start:start + L].copy()
        at = g.choice(L, size=3, replace=False)
        read[at] = (read[at] + 1 + g.integers(0, 3, size=3)) & 3
        strand = int(g.integers(0, 2))
        reads.append(read if strand else (3 - read[::-1]).astype(np.uint8))
        ivs.append((i, 0, strand, 0, L, start, start + L))
        if i < n_hw:
            ancs.append([])
            continue
        j = i - n_hw
        mids = n_nw // n_anch + (1 if j < n_nw % n_anch else 0)
        lone_tail = n_shw % 2 == 1 and j == n_anch - 1      # (an anchor at the read's first base: no head)
        q = np.linspace(0 if lone_tail else 10, L - 10, mids + 1).astype(int)
        assert (np.diff(q) > 0).all()
        ancs.append([(int(x), start + int(x)) for x in q])
    off = np.concatenate([[0], np.cumsum([len(a) for a in ancs])]).astype(np.int64)
    flat = dict(contig_seq=C, contig_off=np.array([0, len(C)], np.int64), read_seq=np.concatenate(reads), read_off=np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64))
    return dict(C=C, reads=reads, ivs=np.array(ivs, np.int64), ancs=ancs, names=["iv%d" % i for i in range(len(ivs))], flat=flat, off=off,
                aq=np.array([q for a in ancs for q, _ in a], np.int32), at=np.array([t for a in ancs for _, t in a], np.int32))


def route_classes(job, pad):
    """(HW, SHW, NW) pieces of the job, counted from the layout"""
    n = [0, 0, 0]
    for iv, a in zip(job["ivs"], job["ancs"]):
        pcs, _, _ = ac.pieces_of(iv, len(job["reads"][iv[0]]), len(job["C"]), [q for q, _ in a], [t for _, t in a], pad)
        for p in pcs:
            if p[0] != "INS":
                n[{"HW": 0, "HEAD": 1, "TAIL": 1, "MID": 2}[p[0]]] += 1
    return tuple(n)
