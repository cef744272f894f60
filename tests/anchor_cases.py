"""The anchor rule (hairsplitter_amd/csrc/hs_map_host.h, "anchors") restated in numpy on top of map_cases / map_split_cases.hits_numpy, the cases that reach
its forks, a small edit-distance DP (NW / SHW / HW) that shares nothing with A1, and the stitched expectation of an interval cut at its anchors.

anchors_of_hits(qa, t, Lr, spacing) is the rule on the best's hits alone, anchors_numpy(p, spacing, contigs, reads) on a whole job; `wrong` swaps one
clause for a plausible mistake, and tests/test_cpu_map_anchors.py shows that the case that claims the fork then gives another result. HIT_CASES are lists of
(qa, t) given as they are: (spacing, Lr, pairs)."""
import bisect
import functools
import subprocess
import tempfile

import numpy as np

import map_cases as mc
import map_split_cases as sc

WRONG = ("non_strict", "both_ascending", "upper_bound", "no_support", "from_previous")
READ_FIELDS = ("n_best", "n_chain", "n_supported")


# ---- the rule ----
def chain_of_hits(qa, t, wrong=None):
    """the ordered hits (qa ascending, t descending) and the canonical chain as indices into them"""
    qa, t = np.asarray(qa, np.int64), np.asarray(t, np.int64)
    o = np.lexsort((t if wrong == "both_ascending" else -t, qa))
    qa, t = qa[o], t[o]
    tails, tail_idx, pred = [], [], []
    search = bisect.bisect_right if wrong in ("upper_bound", "non_strict") else bisect.bisect_left
    for i in range(len(t)):
        at = search(tails, int(t[i]))
        pred.append(tail_idx[at - 1] if at else -1)
        if at == len(tails):
            tails.append(int(t[i])); tail_idx.append(i)
        else:
            tails[at] = int(t[i]); tail_idx[at] = i
    chain = []
    i = tail_idx[-1] if tail_idx else -1
    while i >= 0:
        chain.append(i)
        i = pred[i]
    return qa, t, chain[::-1]


def anchors_of_hits(qa, t, Lr, spacing, wrong=None):
    """dict: q, t (the cut points), n_best, n_chain, n_supported, members (indices into the ordered hits), hits (the ordered (qa, t))"""
    assert spacing >= 1
    qa, t, chain = chain_of_hits(qa, t, wrong)
    d = [int(t[i] - qa[i]) for i in chain]
    sup = [wrong == "no_support" or (j > 0 and d[j - 1] == d[j]) or (j + 1 < len(d) and d[j + 1] == d[j]) for j in range(len(d))]
    cuts, last, prev = [], None, None
    for j, i in enumerate(chain):
        if not sup[j]:
            continue
        ref = prev if wrong == "from_previous" else last
        if last is None or int(qa[i]) - ref >= spacing:
            cuts.append(i)
            last = int(qa[i])
        prev = int(qa[i])
    assert len(cuts) <= Lr // spacing + 1 or wrong is not None
    return dict(q=qa[cuts].astype(np.int64), t=t[cuts].astype(np.int64), n_best=len(qa), n_chain=len(chain), n_supported=int(sum(sup)), members=chain,
                hits=np.stack([qa, t], axis=1) if len(qa) else np.zeros((0, 2), np.int64))


def anchors_numpy(p, spacing, contigs, reads, wrong=None, res=None):
    """every field of hs_map_anchors (anc_off, anc_q, anc_t, n_best, n_chain, n_supported) plus `map` (map_cases.map_numpy's result) and per read `detail`"""
    res = mc.map_numpy(p, contigs, reads) if res is None else res
    ix = res["index"]
    out = {f: np.zeros(len(reads), np.int64) for f in READ_FIELDS}
    off, aq, at, detail = [0], [], [], []
    for r, seq in enumerate(reads):
        d = None
        if res["contig"][r] >= 0 and res["n_hits"][r] <= mc.LDS_CAPACITY:
            H = sc.hits_numpy(p, ix, seq)
            c, rel, b = res["detail"][r]["best"]
            m = (H["c"] == c) & (H["rel"] == rel) & ((H["b"] == b) | (H["b"] == b + 1))
            d = anchors_of_hits(H["qa"][m], H["t"][m], len(seq), spacing, wrong)
            for f in READ_FIELDS:
                out[f][r] = d[f]
            aq += d["q"].tolist(); at += d["t"].tolist()
        detail.append(d)
        off.append(len(aq))
    out.update(anc_off=np.array(off, np.int64), anc_q=np.array(aq, np.int64), anc_t=np.array(at, np.int64), map=res, detail=detail)
    return out


FIELDS = READ_FIELDS + ("anc_off", "anc_q", "anc_t")


def differences(want, got):
    return [f for f in FIELDS if not np.array_equal(np.asarray(want[f], np.int64), np.asarray(got[f], np.int64))]


def inside_interval(res, anc, reads):
    """do the anchors of every read lie inside its interval, ascending strictly in both coordinates?"""
    for r in range(len(reads)):
        q, t = anc["anc_q"][anc["anc_off"][r]:anc["anc_off"][r + 1]], anc["anc_t"][anc["anc_off"][r]:anc["anc_off"][r + 1]]
        if len(q) == 0:
            continue
        Lr = len(reads[r])
        a0, a1 = (res["qstart"][r], res["qend"][r]) if res["strand"][r] else (Lr - res["qend"][r], Lr - res["qstart"][r])
        if res["contig"][r] < 0 or (np.diff(q) <= 0).any() or (np.diff(t) <= 0).any() or q[0] < a0 or q[-1] > a1 or t[0] < res["tstart"][r] or t[-1] > res["tend"][r]:
            return False
    return True


# ---- the selftest harness (tests/harness/map_anchor_selftest.cpp): the C++ host half of the rule ----
def _run(exe, text):
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        f.write(text)
        f.flush()
        return subprocess.run([exe, f.name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def run_harness_hits(exe, spacing, Lr, pairs):
    r = _run(exe, "HITS\n%d %d %d\n" % (spacing, Lr, len(pairs)) + "".join("%d %d\n" % (q, t) for q, t in pairs))
    if r.returncode != 0:
        return dict(returncode=r.returncode, stderr=r.stderr.decode())
    out = dict(returncode=0, members=[], q=[], t=[])
    for line in r.stdout.decode().splitlines():
        f = line.split()
        if f[0] == "A":
            out["n_best"], out["n_chain"], out["n_supported"] = int(f[2]), int(f[3]), int(f[4])
        elif f[0] == "C":
            out["members"].append(int(f[1]))
        elif f[0] == "P":
            out["q"].append(int(f[2])); out["t"].append(int(f[3]))
    return out


def run_harness(exe, p, spacing, contigs, reads, threads=1):
    """the harness's output on a job in the shape of anchors_numpy's result, its map result under `map`"""
    text = "JOB\n%d %d %d %d %d %d %d %d\n%d\n" % (p["k"], p["w"], p["max_occ"], p["band_log2"], p["min_votes"], p["extend"], p["bucket_bits"], threads, spacing)
    for seqs in (contigs, reads):
        text += "%d\n" % len(seqs) + "".join(">" + "".join(map(str, np.asarray(s, np.uint8).tolist())) + "\n" for s in seqs)
    r = _run(exe, text)
    if r.returncode != 0:
        return dict(returncode=r.returncode, stderr=r.stderr.decode())
    res = {f: np.zeros(len(reads), np.int64) for f in mc.FIELDS}
    out = {f: np.zeros(len(reads), np.int64) for f in READ_FIELDS}
    n_anc = np.zeros(len(reads), np.int64)
    aq, at = [], []
    for line in r.stdout.decode().splitlines():
        f = line.split()
        if f[0] == "R":
            for k, v in zip(mc.FIELDS, f[2:]):
                res[k][int(f[1])] = int(v)
        elif f[0] == "A":
            for k, v in zip(READ_FIELDS, f[2:5]):
                out[k][int(f[1])] = int(v)
            n_anc[int(f[1])] = int(f[5])
        elif f[0] == "P":
            aq.append(int(f[2])); at.append(int(f[3]))
    out.update(anc_off=np.concatenate([[0], np.cumsum(n_anc)]).astype(np.int64), anc_q=np.array(aq, np.int64), anc_t=np.array(at, np.int64), map=res, returncode=0)
    return out


# ---- an edit-distance DP of its own: unit costs, rows over the query ----
def edit_distance(q, t, mode):
    """NW: both whole; SHW: the query whole against a prefix of the target; HW: against any stretch of it. Returns the distance."""
    q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
    n = len(t)
    ar = np.arange(n + 1, dtype=np.int64)
    row = np.zeros(n + 1, np.int64) if mode == "HW" else ar.copy()
    for i, c in enumerate(q):
        new = np.empty(n + 1, np.int64)
        new[0] = i + 1
        new[1:] = np.minimum(row[1:] + 1, row[:-1] + (t != c))
        row = np.minimum.accumulate(new - ar) + ar      # (a run of deletions in the row)
    return int(row[-1]) if mode == "NW" else int(row.min())


def read_as_aligned(read, strand):
    return np.asarray(read, np.uint8) if strand else mc.rc(read)


def window_of(contig_len, tstart, tend, pad):
    return max(0, tstart - pad), min(contig_len, tend + pad)


def pieces_of(interval, read_len, contig_len, q, t, pad):
    """the pieces of an interval (read, contig, strand, qstart, qend, tstart, tend) cut at the anchors (q, t): a list of (kind, x0, x1, t0, t1) on the read
    as it aligns and the contig; kinds HW, HEAD, MID, TAIL (handed to the aligner) and INS (a head or tail whose target is empty). Empty heads and tails are
    left out. With it the read range [a0, a1) and the window [w0, w1)."""
    _, _, strand, qs, qe, ts, te = [int(x) for x in interval]
    a0, a1 = (qs, qe) if strand else (read_len - qe, read_len - qs)
    w0, w1 = window_of(contig_len, ts, te, pad)
    out = []
    if len(q) == 0:
        out.append(("HW", a0, a1, w0, w1))
    else:
        if q[0] > a0:
            out.append(("HEAD" if t[0] > w0 else "INS", a0, int(q[0]), w0, int(t[0])))
        for j in range(len(q) - 1):
            out.append(("MID", int(q[j]), int(q[j + 1]), int(t[j]), int(t[j + 1])))
        if q[-1] < a1:
            out.append(("TAIL" if t[-1] < w1 else "INS", int(q[-1]), a1, int(t[-1]), w1))
    return out, (a0, a1), (w0, w1)


def anchored_distance(read, contig, interval, q, t, pad=100):
    """NM of the alignment through the anchors by the DP above, and NM of the HW optimum in the same window"""
    R = read_as_aligned(read, int(interval[2]))
    pcs, (a0, a1), (w0, w1) = pieces_of(interval, len(read), len(contig), q, t, pad)
    nm = 0
    for kind, x0, x1, t0, t1 in pcs:
        if kind == "INS":
            nm += x1 - x0
        elif kind == "HEAD":
            nm += edit_distance(R[x0:x1][::-1], contig[t0:t1][::-1], "SHW")
        else:
            nm += edit_distance(R[x0:x1], contig[t0:t1], {"HW": "HW", "MID": "NW", "TAIL": "SHW"}[kind])
    return nm, edit_distance(R[a0:a1], contig[w0:w1], "HW")


def stitch(pcs, aligned):
    """the record of an interval from its pieces' alignments. aligned[i] = (distance, start, end, moves) of piece i alone, as edlib gives them (a head: of the two
    reversed strings; INS: None). Returns (pos, NM, moves)."""
    moves, nm, pos = [], 0, None
    for (kind, x0, x1, t0, t1), a in zip(pcs, aligned):
        if kind == "INS":
            mv, d = np.ones(x1 - x0, np.uint8), x1 - x0
        else:
            d, start, end, mv = a
            mv = np.asarray(mv, np.uint8)[::-1] if kind == "HEAD" else np.asarray(mv, np.uint8)
        if pos is None:
            pos = t0 + start if kind == "HW" else (t1 - int((mv != 1).sum()) if kind in ("HEAD", "INS") else t0)
        moves.append(mv); nm += d
    return pos, nm, np.concatenate(moves)


def words_of(moves, clip_l, clip_r):
    """the packed CIGAR words of a move string: clips as S (4), '=' and mismatch as M (0), 1 I, 2 D"""
    cls = np.where(moves == 1, 1, np.where(moves == 2, 2, 0))
    cut = np.flatnonzero(np.diff(cls)) + 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(cls)]])
    w = [(clip_l << 4) | 4] if clip_l > 0 else []
    w += [int((e - s) << 4) | int(cls[s]) for s, e in zip(starts, ends)]
    return np.array(w + ([(clip_r << 4) | 4] if clip_r > 0 else []), np.uint32)


def expected_records(api, job, pad):
    """job: C, reads, ivs, ancs (per interval its anchors as (q, t)). Every interval's record from its pieces aligned alone (three calls of api.edlib_align, the entry the committed edlib vectors pin) and stitched in numpy"""
    C, pcs_of, pairs, where = job["C"], [], {"HW": [], "SHW": [], "NW": []}, []
    for iv, a in zip(job["ivs"], job["ancs"]):
        read = job["reads"][iv[0]]
        R = read_as_aligned(read, int(iv[2]))
        pcs, rng, win = pieces_of(iv, len(read), len(C), [q for q, _ in a], [t for _, t in a], pad)
        pcs_of.append((pcs, rng, win))
        for kind, x0, x1, t0, t1 in pcs:
            mode = {"HW": "HW", "HEAD": "SHW", "TAIL": "SHW", "MID": "NW", "INS": None}[kind]
            if mode is None:
                where.append(None)
                continue
            pair = (R[x0:x1][::-1].copy(), C[t0:t1][::-1].copy()) if kind == "HEAD" else (R[x0:x1], C[t0:t1])
            where.append((mode, len(pairs[mode])))
            pairs[mode].append(pair)
    res = {m: api.edlib_align(v, mode=m, task="path") if v else [] for m, v in pairs.items()}
    out, at = [], 0
    for (pcs, (a0, a1), win), iv in zip(pcs_of, job["ivs"]):
        aligned = []
        for _ in pcs:
            w = where[at]; at += 1
            aligned.append(None if w is None else (lambda r: (r["distance"], r["start"], r["end"], r["ops"]))(res[w[0]][w[1]]))
        pos, nm, moves = stitch(pcs, aligned)
        Lr = len(job["reads"][iv[0]])
        out.append(dict(pos=pos, nm=nm, words=words_of(moves, a0, Lr - a1), window=win, n_pieces=sum(p[0] != "INS" for p in pcs)))
    return out


def walk_cigar(words, pos, read, contig, strand, window):
    """a record's CIGAR over the two sequences: (read bases consumed clips included, NM, stays inside the window?)"""
    R = read_as_aligned(read, strand)
    x, t, nm = 0, pos, 0
    inside = pos >= window[0]
    for w in np.asarray(words, np.int64):
        n, op = int(w >> 4), int(w & 15)
        if op == 4:
            x += n
        elif op == 0:
            nm += int((R[x:x + n] != contig[t:t + n]).sum()) if t + n <= len(contig) and x + n <= len(R) else n
            x += n; t += n
        elif op == 1:
            x += n; nm += n
        elif op == 2:
            t += n; nm += n
        else:
            return None
    return x, nm, inside and t <= window[1]


# ---- cases ----
def _hit_cases():
    s = 100
    run = lambda q0, t0, n, step=10: [(q0 + step * i, t0 + step * i) for i in range(n)]
    return {
        # two hits share qa 10: ordered t descending, the later one replaces the earlier; both ascending, both enter the chain
        "equal_qa": (s, 1000, [(10, 100), (10, 300), (20, 400), (30, 500), (40, 510)]),
        # two hits share t 100: the lower-bound search replaces; an upper-bound search (a non-strict chain) keeps both
        "equal_t": (s, 1000, [(10, 100), (20, 100), (30, 200), (40, 210), (50, 220)]),
        # (10, 100) and (20, 50) both lead to (30, 110): the one that was the tail when (30, 110) was placed wins
        "two_longest": (s, 1000, [(10, 100), (20, 50), (30, 110), (40, 120)]),
        "crossing": (s, 1000, run(10, 100, 3) + [(35, 500), (36, 20)] + run(40, 130, 3)),
        # a member alone on its diagonal between two runs: no cut there, although it lies `spacing` behind the first
        "lone_diagonal": (s, 2000, run(10, 100, 2) + [(110, 205)] + run(150, 250, 2)),
        "spacing_edge": (s, 2000, [(0, 50), (s - 1, 50 + s - 1), (s, 50 + s), (2 * s - 1, 50 + 2 * s - 1), (2 * s, 50 + 2 * s)]),
        # 0, 60, 120, 180 on one diagonal: from the last cut 0 and 120; from the previous member never again
        "from_last_cut": (s, 2000, [(0, 50), (60, 110), (120, 170), (180, 230)]),
        "spacing_one": (1, 500, run(5, 40, 6, step=1) + [(20, 60)] + run(30, 80, 3, step=2)),
        "one_hit": (s, 300, [(7, 9)]),
        "descending": (s, 300, [(10, 90), (20, 80), (30, 70)]),
    }


HIT_CASES = _hit_cases()


@functools.lru_cache(maxsize=None)
def want_hits(name):
    s, Lr, pairs = HIT_CASES[name]
    return anchors_of_hits([x[0] for x in pairs], [x[1] for x in pairs], Lr, s)


def _rng(*seed):
    return np.random.default_rng([0x414E] + list(seed))


def _strands():
    """a read of 900 bases and its reverse complement: the same anchors on the read as it aligns"""
    g = _rng(1)
    c = mc._rand(g, 3000)
    r = c[700:1600]
    return mc.params(), 128, [c], [r, mc.rc(r)]


def _unmapped():
    p, contigs, reads = mc.get("unmapped")
    return p, 64, contigs, reads


def _capacity():
    p, contigs, reads = mc.get("capacity")
    return p, 64, contigs, reads


def _lone_seed():
    """a read whose canonical chain holds a seed alone on a foreign diagonal: a word W of the contig lies a second time 30 bases on; the read's copy in
    front and the bases between are spoilt, so no hit lies between the two, and the copy behind hits both: the hit on the first W (the smaller t) takes the
    tail over from the true one. Searched over seeds for a W with one such hit: the rule passes that member over, and without the support rule the cut
    through it costs edits (tests/test_cpu_map_anchors.py). spacing 1: every trusted member is a cut."""
    p = mc.params()
    for seed in range(400):
        g = _rng(2, seed)
        P, W, Q, S = mc._rand(g, 300), mc._rand(g, 18), mc._rand(g, 12), mc._rand(g, 300)
        c = np.concatenate([mc._rand(g, 200), P, W, Q, W, S, mc._rand(g, 200)])
        W2, Q2 = W.copy(), Q.copy()
        W2[::4] = (W2[::4] + 1) & 3
        Q2[[3, 7, 11]] = (Q2[[3, 7, 11]] + 1) & 3
        read = np.concatenate([P, W2, Q2, W, S])
        a = anchors_numpy(p, 1, [c], [read])
        if a["map"]["contig"][0] != 0 or a["n_supported"][0] != a["n_chain"][0] - 1:
            continue
        b = anchors_numpy(p, 1, [c], [read], wrong="no_support", res=a["map"])
        if len(set((a["anc_t"] - a["anc_q"]).tolist())) == 1 and len(set((b["anc_t"] - b["anc_q"]).tolist())) == 2:
            return p, 1, [c], [read]
    raise AssertionError("no read with a seed alone on a foreign diagonal")


CASES = {"strands": _strands, "unmapped": _unmapped, "capacity": _capacity, "lone_seed": _lone_seed}


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def want(name):
    p, spacing, contigs, reads = get(name)
    return anchors_numpy(p, spacing, contigs, reads)


@functools.lru_cache(maxsize=None)
def want_map_case(name, spacing=64):
    """the numpy form on a case of map_cases.CASES"""
    p, contigs, reads = mc.get(name)
    return anchors_numpy(p, spacing, contigs, reads, res=mc.want(name))


@functools.lru_cache(maxsize=None)
def noisy(spacing):
    """test_cpu_map_cases.noisy_case(), default mapper parameters: (the case, params, contigs, the numpy form's anchors)"""
    c = _noisy_case()
    p = mc.params()
    return c, p, [c.seq], anchors_numpy(p, spacing, [c.seq], c.reads, res=_noisy_map())


@functools.lru_cache(maxsize=None)
def _noisy_case():
    from test_cpu_map_cases import noisy_case
    return noisy_case()


@functools.lru_cache(maxsize=None)
def _noisy_map():
    c = _noisy_case()
    return mc.map_numpy(mc.params(), [c.seq], c.reads)
