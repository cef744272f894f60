"""Polishing passes (hairsplitter_amd/csrc/hs_refine_host.h): a numpy restatement of what a pass hands to the next one (where every column
begins in the consensus, the inserted bases in front of it, every piece's window), the composition of entries that the device route is held to, and
the cases. Bundles are those of tests/consensus_cases.py (cc.Bundle, cc.pack, cc.rule); a case's `claim` is worked out by hand from the rule:
  claim["windows"]   the window of every piece after pass 1, (ws, we) in the bundle's consensus, (-1, -1) for none
  claim["passes"]    per pass a dict of fields of that pass's result (cons, n_ins_bases, ...), whichever path the aligner picks."""
import numpy as np

import consensus_cases as cc
import haplotype_cases as hc

SUMS = ("n_sub", "n_del", "n_ins_bases", "n_low", "n_skipped")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def columns_rl(job, min_cov=cc.MIN_COV, max_ins=cc.MAX_INS):
    """columns() with every piece walked in run-length form (cc.piece_runs): for CIGARs whose ops np.repeat cannot hold"""
    return columns(job, min_cov, max_ins, runs=True)


def columns(job, min_cov=cc.MIN_COV, max_ins=cc.MAX_INS, runs=False):
    """col_off [B + 1], col_begin, col_ins (L + 1 entries per bundle), from the rule's text: a column emits its slot's insertion, then one byte unless
    a deletion wins; column t begins where the columns before it end. runs: the votes of a piece come from cc.piece_runs (columns_rl)."""
    col_off, begin, ins_all = [0], [], []
    for b in range(len(job["backbone_off"]) - 1):
        B = job["backbone"][job["backbone_off"][b]:job["backbone_off"][b + 1]]
        L = len(B)
        votes = np.zeros((L, 5), np.int64)
        nins, span = np.zeros(L, np.int64), np.zeros(L, np.int64)
        lens = [[] for _ in range(L)]
        for p in range(job["piece_off"][b], job["piece_off"][b + 1]):
            w = job["cigar"][job["cig_off"][p]:job["cig_off"][p + 1]].astype(np.int64)
            ln, op = w >> 4, w & 15
            text = job["bases"][job["base_off"][p]:job["base_off"][p + 1]]
            s = int(job["piece_sam_pos"][p])
            if len(text) == 0 or (int(job["piece_flags"][p]) & cc.START_BEYOND_SEQ) or int(ln[(op == 0) | (op == 1)].sum()) != len(text) or s - 1 >= L:
                continue
            if runs:
                col_runs, voters = cc.piece_runs(ln, op, s, L)
                for t, n, c, q in col_runs:
                    votes[np.arange(t, t + n), cc._CODE[text[q:q + n]] if c == 0 else 4] += 1
                if col_runs:
                    span[col_runs[0][0] + 1:col_runs[-1][0] + col_runs[-1][1]] += 1
                for slot, src, n in voters:
                    nins[slot] += 1
                    lens[slot].append(min(n, max_ins))
                continue
            ev = np.repeat(op, ln)
            ev = ev[ev <= 2]
            is_col, is_rd = ev != 1, ev != 2
            t = s - 1 + np.cumsum(is_col) - is_col
            q = np.cumsum(is_rd) - is_rd
            ce = np.flatnonzero(is_col & (t < L))
            if len(ce) == 0:
                continue
            code = np.where(ev[ce] == 0, cc._CODE[text[np.minimum(q[ce], len(text) - 1)]], 4)
            np.add.at(votes, (t[ce], code), 1)
            span[t[ce][1:]] += 1
            gaps = np.diff(ce) - 1
            for i in np.flatnonzero(gaps > 0):
                nins[t[ce[i + 1]]] += 1
                lens[int(t[ce[i + 1]])].append(min(int(gaps[i]), max_ins))
        ins = np.zeros(L + 1, np.int64)
        for t in range(1, L):
            if span[t] >= min_cov and 2 * nins[t] > span[t]:
                cnt = np.bincount(np.array(lens[t]), minlength=max_ins + 1)
                ins[t] = int(np.flatnonzero(cnt == cnt.max())[0])
        cov = votes.sum(axis=1)
        ref = cc._CODE[B] if L else np.zeros(0, np.int64)
        top = votes.max(axis=1) if L else np.zeros(0, np.int64)
        ref_tied = votes[np.arange(L), ref] == top if L else np.zeros(0, bool)
        deleted = (cov >= min_cov) & ~ref_tied & (votes[:, :4].max(axis=1) < votes[:, 4]) if L else np.zeros(0, bool)
        out_len = ins[:L] + np.where(deleted, 0, 1)
        begin.append(np.concatenate([[0], np.cumsum(out_len)]))
        ins_all.append(ins)
        col_off.append(col_off[-1] + L + 1)
    cat = lambda x: np.concatenate(x).astype(np.int32) if x else np.zeros(0, np.int32)
    return np.array(col_off, np.int64), cat(begin), cat(ins_all)


def windows(job, col_off, col_begin, col_ins, include_slot=False):
    """win_start, win_end of every piece (hs::refine_window on hc.piece_plan_rl). include_slot: the WRONG rule ws = col_begin[s0]."""
    plan, bundle = hc.piece_plan_rl(job)
    n = len(plan)
    ws, we = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for p in range(n):
        skipped, _, n_cols, _ = (int(x) for x in plan[p])
        if skipped or n_cols < 1:
            continue
        o, s0 = int(col_off[bundle[p]]), int(job["piece_sam_pos"][p]) - 1
        ws[p] = int(col_begin[o + s0]) + (0 if include_slot else int(col_ins[o + s0]))
        we[p] = int(col_begin[o + s0 + n_cols])
    return ws, we


def moves_to_words(moves):
    """run-length words of an alignment in edlib's move codes: 0 and 3 are M, 1 is I, 2 is D"""
    m = np.asarray(moves, np.int64)
    if len(m) == 0:
        return []
    op = np.where(m == 1, 1, np.where(m == 2, 2, 0))
    cut = np.flatnonzero(np.diff(op)) + 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(op)]])
    return [int(((e - s) << 4) | op[s]) for s, e in zip(starts, ends)]


def coded(x):
    return cc._CODE[np.asarray(x, np.uint8)].astype(np.uint8)


def nw_moves(query, target):
    """a plain Needleman-Wunsch with unit costs and SOME traceback (diagonal first): for the claims that hold whichever path is picked"""
    n, m = len(query), len(target)
    D = np.zeros((n + 1, m + 1), np.int64)
    D[:, 0], D[0, :] = np.arange(n + 1), np.arange(m + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i, j] = min(D[i - 1, j - 1] + (query[i - 1] != target[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    i, j, out = n, m, []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (query[i - 1] != target[j - 1]):
            out.append(0 if query[i - 1] == target[j - 1] else 3); i -= 1; j -= 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            out.append(1); i -= 1
        else:
            out.append(2); j -= 1
    return np.array(out[::-1], np.uint8), int(D[n, m])


def next_job(job, prev, ws, we, align):
    """the inputs of the next pass (hs_refine_host.h): prev = a result with cons_off, cons, trim_start, trim_end of the pass before; align(pairs) ->
    [(moves or None, distance)] for pairs of coded arrays. Returns the job, n_pairs, n_unaligned, sum_dist."""
    nb = len(job["backbone_off"]) - 1
    bundle = np.repeat(np.arange(nb), np.diff(job["piece_off"]))
    pairs, at = [], []
    for p in range(len(ws)):
        n_bases = int(job["base_off"][p + 1] - job["base_off"][p])
        if ws[p] >= 0 and we[p] > ws[p] and n_bases > 0:
            o = int(prev["cons_off"][bundle[p]])
            pairs.append((coded(job["bases"][job["base_off"][p]:job["base_off"][p + 1]]), coded(prev["cons"][o + ws[p]:o + we[p]])))
            at.append(p)
    got = dict(zip(at, align(pairs))) if pairs else {}
    cig, cig_off, n_unaligned, sum_dist = [], [0], 0, 0
    for p in range(len(ws)):
        n_bases = int(job["base_off"][p + 1] - job["base_off"][p])
        if p in got:
            moves, dist = got[p]
            if moves is None or len(moves) == 0:
                n_unaligned += 1
            else:
                cig.extend(moves_to_words(moves)); sum_dist += int(dist)
        elif ws[p] >= 0 and we[p] == ws[p] and n_bases > 0:
            cig.append((n_bases << 4) | 1)
        cig_off.append(len(cig))
    lens = np.diff(prev["cons_off"])
    nxt = dict(job)
    nxt.update({"backbone_off": np.asarray(prev["cons_off"], np.int64).copy(), "backbone": np.asarray(prev["cons"], np.uint8).copy(),
                "bundle_overhang_left": np.asarray(prev["trim_start"], np.int32).copy(), "bundle_overhang_right": (lens - prev["trim_end"]).astype(np.int32),
                "piece_sam_pos": np.where(ws < 0, 1, ws + 1).astype(np.int32), "cig_off": np.array(cig_off, np.int64), "cigar": np.array(cig, np.uint32)})
    return nxt, len(pairs), n_unaligned, sum_dist


def compose(job, passes, one_pass, align, params=None):
    """The yardstick: `passes` passes, each one_pass(job, params) -> a result with the keys of api.polish_refine_plan_host. Returns per pass the
    result, and the sums n_pairs, n_unaligned, sum_dist (0 for pass 1)."""
    out, cur = [], job
    counts = (0, 0, 0)
    for p in range(passes):
        res = one_pass(cur, params)
        out.append({"res": res, "n_pairs": counts[0], "n_unaligned": counts[1], "sum_dist": counts[2], "job": cur})
        if p + 1 < passes:
            cur, *counts = next_job(cur, res, res["win_start"], res["win_end"], align)
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
BB = cc.BB
PRE, POST = "CTCATA", "TCATC"


def scattered_cases():
    """the reason for the feature: an indel inside a homopolymer, placed in another slot by every piece"""
    bb, hap = PRE + "GG" + POST, PRE + "GGGG" + POST                 # ...A GG T... against ...A GGGG T...
    ins = [(1, "%dM2I%dM" % (k, 13 - k), hap) for k in (6, 7, 8)]    # the three slots the homopolymer allows
    agree = [(1, "6M2I7M", hap)] * 3
    bb6, hap4 = PRE + "GGGGGG" + POST, PRE + "GGGG" + POST
    dels = [(1, "%dM2D%dM" % (k, 15 - k), hap4) for k in (6, 8, 10)]
    still = {"cons": hap, "n_ins_bases": 0, "n_sub": 0, "n_del": 0}
    return [
        cc.Bundle("a 2-base insertion scattered over three slots", bb, ins, ovl=2, ovr=3,
                  claim={"windows": [(0, 13)] * 3, "passes": [{"cons": bb, "n_ins_bases": 0, "trim_start": 2, "trim_end": 10},
                                                              {"cons": hap, "n_ins_bases": 2, "n_sub": 0, "n_del": 0, "trim_start": 2, "trim_end": 12}, dict(still, trim_end=12)]}),
        cc.Bundle("the same insertion, the three pieces agree on the slot", bb, agree,
                  claim={"windows": [(0, 15)] * 3, "passes": [{"cons": hap, "n_ins_bases": 2}, still, still]}),
        cc.Bundle("a 2-base deletion scattered over three places", bb6, dels,
                  claim={"windows": [(0, 17)] * 3, "passes": [{"cons": bb6, "n_del": 0}, {"cons": hap4, "n_del": 2, "n_sub": 0, "n_ins_bases": 0},
                                                              {"cons": hap4, "n_del": 0, "n_sub": 0, "n_ins_bases": 0}]}),
    ]


def slot_in_front_case():
    """a piece whose first column has a winning insertion in front: ws skips it. Four pieces begin at column 5, three span the slot and insert GG there.
    With the slot's insertion in the window (the WRONG rule) the four align as 2D5M, their deletions outvote the three and pass 2 drops the GG again."""
    c, t = cc._ins(BB, 5, "GG")
    k = BB[:5] + "GG" + BB[5:]
    return cc.Bundle("a winning insertion in front of a piece's first column", BB, [(1, c, t)] * 3 + [(6, "5M", BB[5:])] * 4,
                     claim={"windows": [(0, 12)] * 3 + [(7, 12)] * 4, "wrong_windows": [(0, 12)] * 3 + [(5, 12)] * 4,
                            "passes": [{"cons": k, "n_ins_bases": 2}, {"cons": k, "n_ins_bases": 0, "n_del": 0, "n_sub": 0}], "wrong_pass2": {"cons": BB, "n_del": 2}})


def window_edges_cases():
    full = cc._full(BB, 3)
    dd = (1, "3M1D3M1D2M", BB[:3] + BB[4:7] + BB[8:])                # deletes the columns 3 and 7
    d34 = (1, "3M2D5M", BB[:3] + BB[5:])                             # deletes the columns 3 and 4
    k_dd, k_d34 = BB[:3] + BB[4:7] + BB[8:], BB[:3] + BB[5:]
    a3 = cc._sub(BB, 3, "A")
    return [
        cc.Bundle("pieces at s0 = 0, ending at L - 1 and at L", BB, full + [(1, "9M", BB[:9]), (2, "9M", BB[1:])],
                  claim={"windows": [(0, 10)] * 3 + [(0, 9), (1, 10)], "passes": [{"cons": BB}, {"cons": BB, "n_sub": 0, "n_skipped": 0}]}),
        cc.Bundle("a CIGAR that overruns L", BB, full + [(6, "10M", BB[5:] + "ACGTA")],
                  claim={"windows": [(0, 10)] * 3 + [(5, 10)], "passes": [{"cons": BB}, {"cons": BB}]}),
        slot_in_front_case(),
        cc.Bundle("a piece whose first and last column were deleted", BB, [dd] * 3 + [(4, "5M", BB[3:8])],
                  claim={"windows": [(0, 8)] * 3 + [(3, 6)], "passes": [{"cons": k_dd, "n_del": 2}, {"cons": k_dd, "n_del": 0, "n_skipped": 0}]}),
        cc.Bundle("a piece all of whose columns were deleted", BB, [d34] * 3 + [(4, "2M", BB[3:5])],
                  claim={"windows": [(0, 8)] * 3 + [(3, 3)], "passes": [{"cons": k_d34, "n_del": 2}, {"cons": k_d34, "n_del": 0, "n_skipped": 0}]}),
        cc.Bundle("a piece of I ops only", BB, full + [(4, "3I", "GGG")],
                  claim={"windows": [(0, 10)] * 3 + [(-1, -1)], "passes": [{"cons": BB, "n_skipped": 0}, {"cons": BB, "n_skipped": 1}]}),
        cc.Bundle("the four skipped kinds", BB, cc._full(a3, 3) + [(1, "10M", ""), (1, "10M", BB, cc.START_BEYOND_SEQ), (1, "9M", BB), (11, "1M", "G")],
                  claim={"windows": [(0, 10)] * 3 + [(-1, -1)] * 4, "passes": [{"cons": a3, "n_skipped": 4, "n_sub": 1}, {"cons": a3, "n_skipped": 4, "n_sub": 0}]}),
        cc.Bundle("a bundle without pieces", BB, [], ovl=2, ovr=2,
                  claim={"windows": [], "passes": [{"cons": BB, "n_low": 10, "trim_start": 2, "trim_end": 8}, {"cons": BB, "n_low": 10, "trim_start": 2, "trim_end": 8}]}),
        cc.Bundle("L = 1 and 1-base pieces", "A", cc._full("C", 3), claim={"windows": [(0, 1)] * 3, "passes": [{"cons": "C", "n_sub": 1}, {"cons": "C", "n_sub": 0}]}),
        cc.Bundle("an empty backbone with a piece", "", [(1, "3M", "ACG")], claim={"windows": [(-1, -1)], "passes": [{"cons": "", "n_skipped": 1}, {"cons": "", "n_skipped": 1}]}),
    ]


GATHER_LENGTHS = list(range(1, 18)) + [31, 32, 33, 255, 256, 257, 4095, 4096, 4097]


def gather_edges_cases():
    """every piece length at which the gather takes another path, sibling pieces starting at consecutive columns (every ws mod 16), N and lower-case
    bytes in a piece and in backbone columns that survive under min_cov (4118 .. 4121: covered by fewer than three pieces)"""
    bb = list(cc.seq(4200, 5))
    bb[4119], bb[4121], bb[40] = "N", "a", "n"
    bb = "".join(bb)
    pieces = []
    for i, n in enumerate(GATHER_LENGTHS):
        text = bb[i:i + n]
        if n >= 3:
            text = cc._sub(text, n // 2, cc.other(text[n // 2]))
        if n in (9, 33, 4096):
            text = cc._sub(text, 0, "N")
        if n in (16, 257):
            text = text[:-1] + text[-1].lower()
        pieces.append((i + 1, "%dM" % n, text))
    first = cc.Bundle("a small bundle in front: the next one's text begins at no multiple of 16", BB, cc._full(BB, 3), claim={"windows": [(0, 10)] * 3})
    return [first, cc.Bundle("piece lengths 1 .. 4097 at consecutive columns", bb, pieces, claim={"windows": [(i, i + n) for i, n in enumerate(GATHER_LENGTHS)]})]


def tiers_cases():
    """pieces of 2048 and 2049 bases: A1's grouped kernels and its wave-per-pair kernel, a few substitutions each and one deletion"""
    bb = cc.seq(2100, 8)
    pieces = []
    for j in range(3):
        for n, sam in ((2048, 1), (2049, 11)):
            text = bb[sam - 1:sam - 1 + n]
            for at in (100 + 7 * j, 900 + j, 2000 - j):
                text = cc._sub(text, at, cc.other(text[at]))
            pieces.append((sam, "%dM" % n, text))
    pieces.append((1, "500M1D1547M", bb[:500] + bb[501:2048]))
    return [cc.Bundle("pieces of 2048 and 2049 bases", bb, pieces, claim={"windows": [(0, 2048), (10, 2059)] * 3 + [(0, 2048)]})]


def rounds_cases():
    """more than a megabyte of row bytes: with HS_CONSENSUS_CHUNK_MB=1 at least two sub-rounds, scattered bundles among them"""
    out = []
    for i in range(4):
        bb = cc.seq(6000, 40 + i)
        hap = bb[:3000] + "G" + bb[3000:]
        out.append(cc.Bundle("a bundle of 60 x 6000 row bytes, %d" % i, bb, [(1, "%dM1I%dM" % (2998 + j % 5, 3002 - j % 5), hap) for j in range(60)]))
        out.extend(scattered_cases())
    return out


def a1_chunks_cases(n_bundles=8, n_pieces=300, L=4000):
    """Queries plus windows of one sub-round above 16 MiB (8 x 300 pairs of 4001 + 4000 bases: 19.2 MB), so that A1 under HS_REALIGN_CHUNK_MB=16 (the
    floor) runs in two chunks. In the style of rounds_cases: piece j carries the haplotype's one inserted base at 1998 + j mod 5, no slot wins pass 1,
    pass 2 finds the haplotype. Returns (bundles, the haplotypes)."""
    out, haps = [], []
    for i in range(n_bundles):
        bb = cc.seq(L, 60 + i)
        hap = bb[:L // 2] + "G" + bb[L // 2:]
        out.append(cc.Bundle("a bundle of %d pieces of %d bases, %d" % (n_pieces, L + 1, i), bb,
                             [(1, "%dM1I%dM" % (L // 2 - 2 + j % 5, L - (L // 2 - 2 + j % 5)), hap) for j in range(n_pieces)]))
        haps.append(hap)
    return out, haps


CASES = {"scattered": scattered_cases, "window_edges": window_edges_cases, "gather_edges": gather_edges_cases, "tiers": tiers_cases}


def _true_cigar(events):
    """run-length words of a string of M, I and D characters"""
    chars = np.frombuffer(events.encode(), np.uint8)
    cut = np.flatnonzero(np.diff(chars)) + 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(chars)]])
    return [int(((e - s) << 4) | "MID".index(chr(chars[s]))) for s, e in zip(starts, ends)]


def noisy_cases(seed=5, n_pieces=12, hap_len=1040, piece_len=1000):
    """Outside CASES (the CPU claims test runs a Python Needleman-Wunsch over those): two bundles of 12 seeded pieces of about 1000 bases. Every
    piece has 8 % isolated errors of its own against its bundle's haplotype -- odd pieces 1 % substitutions and 7 % 1-base insertions and deletions,
    even ones 4 % and 4 % -- and the backbone differs from the haplotype by three indels. Starts are staggered over 0 .. 40, the CIGARs of pass 1
    are the true ones. Pass 2 then reads CIGARs the device wrote, of some 80 and some 140 words: beyond one and beyond two 64-op chunks."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2):
        hap = cc.seq(hap_len, 500 + k)
        gone, extra = {300 + k: True, 901: True}, {600: "T"}      # haplotype bases the backbone lacks; backbone bases in front of a haplotype base
        bb, col_of = [], []
        for i, c in enumerate(hap):
            bb.append(extra.get(i, ""))
            col_of.append(sum(len(x) for x in bb))
            if i not in gone:
                bb.append(c)
        bb = "".join(bb)
        pieces = []
        for j in range(n_pieces):
            a = (j * 40) // (n_pieces - 1)
            b = min(hap_len, a + piece_len)
            p_sub, p_indel = (0.01, 0.07) if j % 2 else (0.04, 0.04)
            kind = np.zeros(hap_len, np.int64)      # 0 none, 1 substitution, 2 the base is missing, 3 an inserted base in front
            draw = rng.random(hap_len)
            kind[draw < p_sub] = 1
            kind[(draw >= p_sub) & (draw < p_sub + p_indel / 2)] = 2
            kind[(draw >= p_sub + p_indel / 2) & (draw < p_sub + p_indel)] = 3
            for i in range(hap_len):                # isolated, away from the piece's ends and from the backbone's own indels
                near = any(abs(i - x) <= 2 for x in list(gone) + list(extra))
                if kind[i] and (i < a + 3 or i >= b - 3 or near or kind[i - 1]):
                    kind[i] = 0
            text, ev = [], []
            for i in range(a, b):
                if i in extra:
                    ev.append("D" * len(extra[i]))
                if kind[i] == 3:
                    text.append("ACGT"[int(rng.integers(4))]); ev.append("I")
                if kind[i] == 2:
                    ev.append("D")
                else:
                    text.append(cc.other(hap[i]) if kind[i] == 1 else hap[i]); ev.append("I" if i in gone else "M")
            pieces.append((col_of[a] + 1, _true_cigar("".join(ev)), "".join(text)))
        out.append(cc.Bundle("noisy bundle %d" % k, bb, pieces, ovl=20, ovr=25))
    return out


NOISY = {"noisy": noisy_cases}


def check_windows(bundles, job, ws, we, key="windows"):
    for i, b in enumerate(bundles):
        if key in b.claim:
            p0, p1 = int(job["piece_off"][i]), int(job["piece_off"][i + 1])
            assert list(zip(ws[p0:p1].tolist(), we[p0:p1].tolist())) == [tuple(x) for x in b.claim[key]], (b.name, key)


def check_pass_claims(bundles, p, res):
    """the claims of pass p (1-based) against a result with the keys of api.polish_consensus"""
    got = cc.result_as_rule(res) if "stats" in res else res
    for i, b in enumerate(bundles):
        claims = b.claim.get("passes", [])
        if p - 1 < len(claims):
            for k, v in claims[p - 1].items():
                have = got["cons"][i].decode() if k == "cons" else got[k][i]
                assert have == v, (b.name, "pass", p, k, have, v)
