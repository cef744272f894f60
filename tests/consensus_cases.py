"""The bundle consensus (hairsplitter_amd/csrc/hs_consensus_host.h): a numpy restatement of the rule and the cases that hold the
C++ host half (tests/test_cpu_consensus.py) and the device (tests/test_gpu_consensus.py) to it. Bundles are built from explicit CIGARs; the two
sides of every fork are sibling bundles of one call. A case's `claim` is what its fork must come to, worked out by hand from the rule."""
import re

import numpy as np

MIN_COV, MAX_INS = 3, 32      # the defaults of hs_consensus_params (placeholders)
START_BEYOND_SEQ = 2          # HS_POLISH_START_BEYOND_SEQ
OPS = "MIDNSHP=X"
FIELDS = ("trim_start", "trim_end", "n_sub", "n_del", "n_ins_bases", "n_low", "n_skipped")
WRONG_RULES = ("tie_lowest", "slot_ge", "leading_ins", "tie_longer", "exact_length", "cov_m_only")


def words(cigar):
    """'3M2I' -> [len << 4 | op]"""
    return [(int(n) << 4) | OPS.index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def seq(n, seed=1):
    """n letters, the same on every call"""
    x, out = 12345 + seed, []
    for _ in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4] if c in "ACGT" else "A"


class Bundle:
    def __init__(self, name, backbone, pieces, ovl=0, ovr=0, claim=None):
        """pieces: (sam_pos, cigar string or word list, text[, flags])"""
        self.name, self.backbone, self.ovl, self.ovr, self.claim = name, backbone, ovl, ovr, dict(claim or {})
        self.pieces = [(p[0], words(p[1]) if isinstance(p[1], str) else list(p[1]), p[2], p[3] if len(p) > 3 else 0) for p in pieces]


def pack(bundles):
    """the arrays of hs_polish_consensus_arrays (the keys of api.polish_consensus)"""
    bb, bases, cig = [], [], []
    out = {"backbone_off": [0], "piece_off": [0], "base_off": [0], "cig_off": [0], "bundle_overhang_left": [], "bundle_overhang_right": [], "piece_sam_pos": [], "piece_flags": []}
    for b in bundles:
        bb.append(b.backbone)
        out["backbone_off"].append(out["backbone_off"][-1] + len(b.backbone))
        out["bundle_overhang_left"].append(b.ovl)
        out["bundle_overhang_right"].append(b.ovr)
        for sam, w, text, flags in b.pieces:
            bases.append(text)
            cig.extend(w)
            out["piece_sam_pos"].append(sam)
            out["piece_flags"].append(flags)
            out["base_off"].append(out["base_off"][-1] + len(text))
            out["cig_off"].append(len(cig))
        out["piece_off"].append(len(out["piece_sam_pos"]))
    res = {k: np.array(v, np.int64 if k.endswith("_off") else np.int32) for k, v in out.items()}
    res["backbone"] = np.frombuffer("".join(bb).encode(), np.uint8).copy()
    res["bases"] = np.frombuffer("".join(bases).encode(), np.uint8).copy()
    res["cigar"] = np.array(cig, np.uint32)
    return res


_CODE = np.full(256, 3, np.int64)
_CODE[ord("A")], _CODE[ord("C")], _CODE[ord("G")] = 0, 1, 2
_LETTER = np.frombuffer(b"ACGT", np.uint8)


def piece_runs(ln, op, s, L):
    """The walk of one piece in run-length form, from the rule's text (hs_consensus_host.h: walk, slot): every op is clipped at the room left
    (L - t) BEFORE anything per event exists, so a piece costs O(ops), whatever its lengths (an op holds up to 2^28 - 1 events).
    Returns (runs, ins): runs = [(t, n, op, q)], the column ops inside the room -- n >= 1 events from column t on, the read cursor q at the first;
    ins = [(slot, src, n)], the insertions that vote -- n inserted bases from read offset src, in front of column `slot`, a column event before."""
    t, q, pending, src, runs, ins = int(s) - 1, 0, 0, 0, [], []
    for n, c in zip((int(x) for x in ln), (int(x) for x in op)):
        if t >= L:
            break
        if n == 0 or c > 2:
            continue
        if c == 1:
            if pending == 0:
                src = q
            pending += n
            q += n
            continue
        if pending and runs:
            ins.append((t, src, pending))
        pending = 0
        k = min(n, L - t)
        runs.append((t, k, c, q))
        t += k
        if c == 0:
            q += n
    return runs, ins


def rule_rl(job, min_cov=MIN_COV, max_ins=MAX_INS):
    """rule() with every piece walked in run-length form (piece_runs): for CIGARs whose ops np.repeat cannot hold"""
    return rule(job, min_cov, max_ins, runs=True)


def rule(job, min_cov=MIN_COV, max_ins=MAX_INS, wrong=None, runs=False):
    """The rule in numpy, bundle by bundle: {"cons": [bytes per bundle], FIELDS: lists, "n_ins_records", "n_ins_slots"}.
    wrong: one of WRONG_RULES -- a deliberately wrong rule, which the case that claims the fork must tell from the right one.
    runs: the votes of a piece come from piece_runs() instead of one array entry per event (rule_rl); the decisions are the same lines."""
    assert not (runs and wrong)
    out = {k: [] for k in FIELDS}
    out["cons"] = []
    n_records = n_slots = 0
    for b in range(len(job["backbone_off"]) - 1):
        B = job["backbone"][job["backbone_off"][b]:job["backbone_off"][b + 1]]
        L = len(B)
        votes = np.zeros((L, 5), np.int64)
        nins, span = np.zeros(L, np.int64), np.zeros(L, np.int64)
        ins = [[] for _ in range(L)]      # per slot: the (capped) insertions of its voters
        skipped = 0
        for p in range(job["piece_off"][b], job["piece_off"][b + 1]):
            w = job["cigar"][job["cig_off"][p]:job["cig_off"][p + 1]].astype(np.int64)
            ln, op = w >> 4, w & 15
            text = job["bases"][job["base_off"][p]:job["base_off"][p + 1]]
            s = int(job["piece_sam_pos"][p])
            if len(text) == 0 or (int(job["piece_flags"][p]) & START_BEYOND_SEQ) or int(ln[(op == 0) | (op == 1)].sum()) != len(text) or s - 1 >= L:
                skipped += 1
                continue
            if runs:
                col_runs, voters = piece_runs(ln, op, s, L)
                for t, n, c, q in col_runs:
                    votes[np.arange(t, t + n), _CODE[text[q:q + n]] if c == 0 else 4] += 1
                if col_runs:
                    span[col_runs[0][0] + 1:col_runs[-1][0] + col_runs[-1][1]] += 1
                for slot, src, n in voters:
                    nins[slot] += 1
                    ins[slot].append(text[src:src + min(n, max_ins)])
                    n_records += 1
                continue
            ev = np.repeat(op, ln)
            ev = ev[ev <= 2]                       # one entry per M, I or D char; nothing else moves a cursor
            is_col, is_rd = ev != 1, ev != 2
            t = s - 1 + np.cumsum(is_col) - is_col
            q = np.cumsum(is_rd) - is_rd
            ce = np.flatnonzero(is_col & (t < L))  # the column events of the walk (it ends at the first t >= L)
            if len(ce) == 0:
                continue
            code = np.where(ev[ce] == 0, _CODE[text[np.minimum(q[ce], len(text) - 1)]], 4)
            np.add.at(votes, (t[ce], code), 1)
            span[t[ce][1:]] += 1
            gaps = np.diff(ce) - 1                 # between two column events there are only I chars
            for i in np.flatnonzero(gaps > 0):
                slot, src, n = int(t[ce[i + 1]]), int(q[ce[i] + 1]), int(gaps[i])
                nins[slot] += 1
                ins[slot].append(text[src:src + min(n, max_ins)])
                n_records += 1
            if wrong == "leading_ins" and ce[0] > 0:
                nins[t[ce[0]]] += 1
                ins[t[ce[0]]].append(text[:min(int(ce[0]), max_ins)])
        cons = bytearray()
        n_sub = n_del = n_ib = n_low = 0
        c_start, c_end = min(int(job["bundle_overhang_left"][b]), L), L - min(int(job["bundle_overhang_right"][b]), L)
        trim = {}
        for t in range(L):
            if t == c_start:
                trim["s"] = len(cons)
            if t == c_end:
                trim["e"] = len(cons)
            wins = span[t] >= min_cov and (2 * nins[t] >= span[t] if wrong == "slot_ge" else 2 * nins[t] > span[t])
            if t >= 1 and wins and len(ins[t]):
                n_slots += 1
                lens = np.array([len(x) for x in ins[t]])
                cnt = np.bincount(lens, minlength=max_ins + 1)
                tied = np.flatnonzero(cnt == cnt.max())
                ell = int(tied[-1] if wrong == "tie_longer" else tied[0])
                for j in range(ell):
                    col = [x[j] for x in ins[t] if (len(x) == ell if wrong == "exact_length" else len(x) > j)]
                    cons.append(_LETTER[int(np.argmax(np.bincount(_CODE[np.array(col)], minlength=4)))])
                n_ib += ell
            v = votes[t]
            cov = int(v[:4].sum()) if wrong == "cov_m_only" else int(v.sum())
            if cov < min_cov:
                n_low += 1
                cons.append(B[t])
                continue
            ref = int(_CODE[B[t]])
            tied = np.flatnonzero(v == v.max())
            win = ref if (ref in tied and wrong != "tie_lowest") else int(tied[0])
            if win == 4:
                n_del += 1
            else:
                cons.append(_LETTER[win])
                n_sub += win != ref
        trim.setdefault("s", len(cons))
        trim.setdefault("e", len(cons))
        if c_start == L:
            trim["s"] = len(cons)
        if c_end == L:
            trim["e"] = len(cons)
        out["cons"].append(bytes(cons))
        for k, x in zip(FIELDS, (trim["s"], trim["e"], n_sub, n_del, n_ib, n_low, skipped)):
            out[k].append(int(x))
    out["n_ins_records"], out["n_ins_slots"] = n_records, n_slots
    return out


def result_as_rule(res):
    """a result of api.polish_consensus in the shape rule() returns"""
    out = {k: [int(x) for x in res[k]] for k in FIELDS}
    out["cons"] = [res["cons"][int(res["cons_off"][i]):int(res["cons_off"][i + 1])].tobytes() for i in range(len(res["cons_off"]) - 1)]
    out["n_ins_records"], out["n_ins_slots"] = res["stats"]["n_ins_records"], res["stats"]["n_ins_slots"]
    return out


def write_job(path, job, min_cov=MIN_COV, max_ins=MAX_INS, threads=1):
    """the text tests/harness/consensus_selftest reads"""
    nb = len(job["backbone_off"]) - 1
    lines = ["%d %d %d" % (min_cov, max_ins, threads), str(nb)]
    for b in range(nb):
        bb = job["backbone"][job["backbone_off"][b]:job["backbone_off"][b + 1]].tobytes().decode()
        p0, p1 = int(job["piece_off"][b]), int(job["piece_off"][b + 1])
        lines.append("B %d %d %d %s" % (job["bundle_overhang_left"][b], job["bundle_overhang_right"][b], p1 - p0, bb or "-"))
        for p in range(p0, p1):
            w = job["cigar"][job["cig_off"][p]:job["cig_off"][p + 1]]
            text = job["bases"][job["base_off"][p]:job["base_off"][p + 1]].tobytes().decode()
            lines.append("P %d %d %d %s %s" % (job["piece_sam_pos"][p], job["piece_flags"][p], len(w), " ".join(str(int(x)) for x in w), text or "-"))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def parse_selftest(stdout):
    out = {k: [] for k in FIELDS}
    out["cons"] = []
    for line in stdout.splitlines():
        f = line.split()
        if f[0] == "C":
            for k, x in zip(FIELDS, f[2:9]):
                out[k].append(int(x))
            out["cons"].append(b"" if f[9] == "-" else f[9].encode())
        elif f[0] == "T":
            out["n_ins_records"], out["n_ins_slots"] = int(f[1]), int(f[2])
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
BB = "ACGTACGTAC"      # the backbone of the small cases: column 3 is T, column 9 is C


def _sub(text, at, c):
    return text[:at] + c + text[at + 1:]


def _full(text, n, cigar=None, sam=1):
    return [(sam, cigar or "%dM" % len(text), text)] * n


def columns_cases():
    a3, c3, g3 = _sub(BB, 3, "A"), _sub(BB, 3, "C"), _sub(BB, 3, "G")
    d3 = (1, "3M1D6M", BB[:3] + BB[4:])
    bn = _sub(BB, 3, "N")
    return [
        Bundle("cov = min_cov - 1", BB, _full(a3, 2), claim={"n_low": 10, "n_sub": 0, "cons": BB}),
        Bundle("cov = min_cov", BB, _full(a3, 3), claim={"n_low": 0, "n_sub": 1, "cons": a3}),
        Bundle("2:2, the backbone base tied", BB, _full(BB, 2) + _full(a3, 2), claim={"n_sub": 0, "cons": BB}),
        Bundle("2:2, the backbone base not tied", BB, _full(c3, 2) + _full(g3, 2), claim={"n_sub": 1, "cons": c3}),
        Bundle("2:2, deletion tied with a base, the backbone's not", BB, [d3, d3] + _full(a3, 2), claim={"n_sub": 1, "n_del": 0, "cons": a3}),
        Bundle("2:2, deletion tied with the backbone base", BB, [d3, d3] + _full(BB, 2), claim={"n_sub": 0, "n_del": 0, "cons": BB}),
        Bundle("a deletion majority", BB, [d3, d3, d3] + _full(BB, 1), claim={"n_del": 1, "cons": BB[:3] + BB[4:]}),
        Bundle("two deletions and a base: covered by three", BB, [d3, d3] + _full(BB, 1), claim={"n_del": 1, "n_low": 0, "cons": BB[:3] + BB[4:]}),
        Bundle("a byte outside ACGT votes as T", bn, _full(bn, 3), claim={"n_sub": 0, "n_low": 0, "cons": BB}),
        Bundle("a byte outside ACGT is kept below min_cov", bn, _full(bn, 2), claim={"n_low": 10, "cons": bn}),
    ]


def _ins(text, at, s):
    """(cigar, text) of a piece over all of `text` with s inserted in front of column at"""
    return "%dM%dI%dM" % (at, len(s), len(text) - at), text[:at] + s + text[at:]


def slots_cases():
    def piece(s, at=5):
        c, t = _ins(BB, at, s)
        return (1, c, t)
    lead = (3, "2I6M1I", "GG" + BB[2:8] + "G")
    g32, g33 = seq(32, 7), seq(33, 7)
    return [
        Bundle("2 nins = span", BB, [piece("G")] * 2 + _full(BB, 2), claim={"n_ins_bases": 0, "cons": BB}),
        Bundle("2 nins = span + 1", BB, [piece("G")] * 3 + _full(BB, 2), claim={"n_ins_bases": 1, "cons": BB[:5] + "G" + BB[5:]}),
        Bundle("span = min_cov - 1, every piece inserts", BB, [piece("G")] * 2, claim={"n_ins_bases": 0, "n_low": 10, "cons": BB}),
        Bundle("span = min_cov, every piece inserts", BB, [piece("G")] * 3, claim={"n_ins_bases": 1, "cons": BB[:5] + "G" + BB[5:]}),
        Bundle("a leading and a trailing I vote nowhere", BB, [lead] * 3 + _full(BB, 3), claim={"n_ins_bases": 0, "cons": BB}),
        Bundle("I at slot 1 and at slot L - 1", BB, [(1, "1M1I8M1I1M", BB[0] + "G" + BB[1:9] + "T" + BB[9])] * 3,
               claim={"n_ins_bases": 2, "cons": BB[0] + "G" + BB[1:9] + "T" + BB[9]}),
        Bundle("2I 3I back to back: one insertion", BB, [(1, "5M2I3I5M", BB[:5] + "GGTTT" + BB[5:])] * 3, claim={"n_ins_bases": 5, "cons": BB[:5] + "GGTTT" + BB[5:]}),
        Bundle("2I 1N 3I: one insertion", BB, [(1, "5M2I1N3I5M", BB[:5] + "GGTTT" + BB[5:])] * 3, claim={"n_ins_bases": 5, "cons": BB[:5] + "GGTTT" + BB[5:]}),
        Bundle("a length tie: the shorter", BB, [piece("G")] * 2 + [piece("GT")] * 2, claim={"n_ins_bases": 1, "cons": BB[:5] + "G" + BB[5:]}),
        Bundle("lengths 1, 2, 3 vote per offset", BB, [piece("C"), piece("CA"), piece("GAT"), piece("GAT")], claim={"n_ins_bases": 3, "cons": BB[:5] + "CAT" + BB[5:]}),
        Bundle("length max_ins", BB, [piece(g32)] * 3, claim={"n_ins_bases": 32, "cons": BB[:5] + g32 + BB[5:]}),
        Bundle("length max_ins + 1", BB, [piece(g33)] * 3, claim={"n_ins_bases": 32, "cons": BB[:5] + g32 + BB[5:]}),
    ]


def _pattern_cigar(n_ops):
    """n_ops ops 3M 1I 2M 1D ... ending in M, with the text of a piece that follows `backbone` but for a wrong last base"""
    pat = [(3, "M"), (1, "I"), (2, "M"), (1, "D")]
    ops = [pat[i % 4] for i in range(n_ops)]
    if ops[-1][1] != "M":
        ops[-1] = (2, "M")
    return ops


def _follow(backbone, ops, at=0):
    """the text of a piece that walks `ops` from column `at` and agrees with the backbone; inserted bases are G"""
    text, t = [], at
    for n, c in ops:
        if c == "M":
            text.append("".join(backbone[u] if u < len(backbone) else "A" for u in range(t, t + n)))
            t += n
        elif c == "D":
            t += n
        elif c == "I":
            text.append("G" * n)
    return "".join(text), t - at


def edges_cases():
    out = []
    for L in (1, 2, 255, 256, 257, 513):
        bb = seq(L, L)
        wrong = _sub(bb, L - 1, other(bb[L - 1]))
        out.append(Bundle("L = %d" % L, bb, _full(wrong, 3), claim={"n_sub": 1, "n_low": 0, "cons": wrong}))
    bb = seq(513, 3)
    first = other(bb[255]) + bb[256:265]
    out.append(Bundle("a piece that starts on a tile's last column", bb, _full(first, 3, sam=256), claim={"n_sub": 1, "n_low": 503, "cons": bb[:255] + first + bb[265:]}))
    out.append(Bundle("a D and an M op across a tile edge", bb, [(250, "4M6D4M", bb[249:253] + bb[259:263])] * 3, claim={"n_del": 6, "n_low": 499, "cons": bb[:253] + bb[259:]}))
    out.append(Bundle("a winning slot at t = 256", bb, [(250, "7M2I7M", bb[249:256] + "GT" + bb[256:263])] * 3,
                      claim={"n_ins_bases": 2, "n_low": 499, "cons": bb[:256] + "GT" + bb[256:]}))
    bb = seq(300, 4)
    end = bb[290:299] + other(bb[299])
    out.append(Bundle("a piece that ends on L", bb, _full(end, 3, sam=291), claim={"n_sub": 1, "n_low": 290, "cons": bb[:290] + end}))
    out.append(Bundle("a piece that overruns L by 17", bb, _full(end + seq(17, 5), 3, sam=291), claim={"n_sub": 1, "n_low": 290, "n_skipped": 0, "cons": bb[:290] + end}))
    out.append(Bundle("s - 1 = L - 1", BB, _full("G", 3, sam=10), claim={"n_sub": 1, "n_low": 9, "n_skipped": 0, "cons": BB[:9] + "G"}))
    out.append(Bundle("s - 1 = L", BB, _full("G", 3, sam=11), claim={"n_sub": 0, "n_low": 10, "n_skipped": 3, "cons": BB}))
    for n_ops in (64, 65, 128, 129):
        ops = _pattern_cigar(n_ops)
        bb = seq(260, n_ops)
        text, cols = _follow(bb, ops)
        n_d = sum(n for n, c in ops if c == "D")
        n_i = sum(n for n, c in ops[:-1] if c == "I")
        out.append(Bundle("a CIGAR of %d ops" % n_ops, bb, [(1, [(n << 4) | OPS.index(c) for n, c in ops], text)] * 3,
                          claim={"n_del": n_d, "n_ins_bases": n_i, "n_sub": 0, "n_low": 260 - cols}))
    ops = [(15, "M"), (1, "I"), (16, "M"), (1, "D"), (17, "M"), (2, "I"), (33, "M"), (15, "D"), (1, "M"), (16, "D"), (1, "M"), (17, "D"), (1, "M"), (33, "D"), (2, "M")]
    bb = seq(200, 9)
    text, cols = _follow(bb, ops, at=5)
    out.append(Bundle("ops of 15, 16, 17 and 33 events", bb, [(6, [(n << 4) | OPS.index(c) for n, c in ops], text)] * 3,
                      claim={"n_del": 1 + 15 + 16 + 17 + 33, "n_ins_bases": 3, "n_sub": 0, "n_low": 200 - cols}))
    return out


def pieces_cases():
    a3 = _sub(BB, 3, "A")
    good = _full(a3, 3)
    inert = (1, "3M2=2X1N1P7M", a3)
    out = [
        Bundle("an empty piece", BB, good + [(1, "10M", "")], claim={"n_skipped": 1, "n_sub": 1, "cons": a3}),
        Bundle("a flagged piece", BB, good + [(1, "10M", BB, START_BEYOND_SEQ)], claim={"n_skipped": 1, "n_sub": 1, "cons": a3}),
        Bundle("sum(M + I) differs from the bases", BB, good + [(1, "9M", BB), (1, "9M2I", BB)], claim={"n_skipped": 2, "n_sub": 1, "cons": a3}),
        Bundle("= X N P inside a CIGAR move nothing", BB, [inert] * 3, claim={"n_skipped": 0, "n_sub": 1, "n_low": 0, "cons": a3}),
        Bundle("a bundle without pieces", BB, [], ovl=2, ovr=2, claim={"n_low": 10, "cons": BB, "trim_start": 2, "trim_end": 8}),
        Bundle("an empty backbone", "", [], claim={"cons": "", "trim_start": 0, "trim_end": 0}),
        Bundle("an empty backbone with a piece", "", [(1, "3M", "ACG")], claim={"cons": "", "n_skipped": 1}),
        Bundle("a depth of 300", "ACGT", _full("ACTT", 151) + _full("ACGT", 149), claim={"n_sub": 1, "cons": "ACTT"}),
    ]
    return out


def many_cases(n):
    """n small bundles in one call, every other one with a substitution"""
    out = []
    for i in range(n):
        bb = seq(5 + i % 7, 100 + i)
        text = _sub(bb, 2, other(bb[2])) if i % 2 else bb
        out.append(Bundle("bundle %d of %d" % (i, n), bb, _full(text, 3), claim={"n_sub": i % 2, "cons": text}))
    return out


def trim_cases():
    dd = (1, "3M1D3M1D2M", BB[:3] + BB[4:7] + BB[8:])
    ii = (1, "3M1I4M1I3M", BB[:3] + "G" + BB[3:7] + "G" + BB[7:])
    return [
        Bundle("overhangs 0", BB, _full(BB, 3), claim={"trim_start": 0, "trim_end": 10}),
        Bundle("overhang left L", BB, _full(BB, 3), ovl=10, claim={"trim_start": 10, "trim_end": 10}),
        Bundle("overhang right L", BB, _full(BB, 3), ovr=10, claim={"trim_start": 0, "trim_end": 0}),
        Bundle("a deletion at either overhang column", BB, [dd] * 3, ovl=3, ovr=3, claim={"n_del": 2, "trim_start": 3, "trim_end": 6, "cons": BB[:3] + BB[4:7] + BB[8:]}),
        Bundle("a winning slot at either overhang column", BB, [ii] * 3, ovl=3, ovr=3, claim={"n_ins_bases": 2, "trim_start": 3, "trim_end": 8}),
    ]


CASES = {"columns": columns_cases, "slots": slots_cases, "edges": edges_cases, "pieces": pieces_cases, "many65": lambda: many_cases(65), "many129": lambda: many_cases(129),
         "trim": trim_cases}
# the case that tells each wrong rule from the right one: (group, bundle name)
WRONG_RULE_CASE = {"tie_lowest": ("columns", "2:2, the backbone base tied"), "slot_ge": ("slots", "2 nins = span"), "leading_ins": ("slots", "a leading and a trailing I vote nowhere"),
                   "tie_longer": ("slots", "a length tie: the shorter"), "exact_length": ("slots", "lengths 1, 2, 3 vote per offset"),
                   "cov_m_only": ("columns", "two deletions and a base: covered by three")}


def check_claims(bundles, got):
    """every fork a case claims, from the fields of a result in rule()'s shape"""
    for i, b in enumerate(bundles):
        for k, v in b.claim.items():
            have = got["cons"][i].decode() if k == "cons" else got[k][i]
            assert have == v, (b.name, k, have, v)


def assert_same(a, b, what=""):
    for k in FIELDS + ("cons", "n_ins_records", "n_ins_slots"):
        assert a[k] == b[k], (what, k)
