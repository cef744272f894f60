"""The split mapper's rule (hairsplitter_amd/csrc/hs_map_host.h, "split mappings"), restated in numpy on top of map_cases.minimizers / index_numpy, and
the cases that reach its forks.

split_numpy(p, sp, contigs, reads) shares nothing with the C++ but the specification; `wrong` swaps one clause for a plausible mistake, and
tests/test_cpu_map_split.py shows that the case that claims the fork then gives another result. A case is (params, split params, contigs, reads);
truth, where a case has one, is a list of (read, contig, strand, qstart, qend, tstart, tend). CASES lists them; get(name) builds one (cached)."""
import functools
import subprocess
import tempfile

import numpy as np

import map_cases as mc

SPLIT_DEFAULT = dict(max_segments=4, min_votes=3, min_span=100, max_gap=200)
SEG_FIELDS = ("read", "contig", "strand", "qstart", "qend", "tstart", "tend", "votes", "second", "round")
READ_FIELDS = ("n_minimizers", "n_hits", "n_skipped", "read_votes", "read_second")
WRONG = ("overlap_one", "no_gap", "rightmost_gap", "always_extend", "skip", "index_min_votes")
rc, params = mc.rc, mc.params


def split(**kw):
    s = dict(SPLIT_DEFAULT)
    s.update(kw)
    return s


def split_valid(s):
    return 1 <= s["max_segments"] <= 8 and s["min_votes"] >= 1 and s["min_span"] >= 0 and s["max_gap"] >= 0


def hits_numpy(p, ix, seq):
    """the hits of one read: q (k-mer start on the read as given), qa, t, contig, rel, bin; the read's minimizer counts"""
    k, Lr = p["k"], len(seq)
    pos, h, s = mc.minimizers(seq, k, p["w"])
    lo = np.searchsorted(ix["h"], h, "left"); hi = np.searchsorted(ix["h"], h, "right")
    occ = hi - lo
    keep = occ <= p["max_occ"]
    rep = np.where(keep, occ, 0)
    e = (np.repeat(lo, rep) + (np.arange(rep.sum()) - np.repeat(np.cumsum(rep) - rep, rep))).astype(np.int64)
    q = np.repeat(pos, rep).astype(np.int64)
    rel = np.repeat(s, rep).astype(np.int64) ^ ix["s"][e].astype(np.int64)
    t = ix["t"][e]
    qa = np.where(rel == 1, Lr - k - q, q)
    return dict(q=q, qa=qa, t=t, c=ix["c"][e], rel=rel, b=(t - qa + Lr) >> p["band_log2"], n_minimizers=len(pos), n_skipped=int((~keep).sum()))


def _scores(H, m):
    n = {}
    for key in zip(H["c"][m].tolist(), H["rel"][m].tolist(), H["b"][m].tolist()):
        n[key] = n.get(key, 0) + 1
    return {key: v + n.get((key[0], key[1], key[2] + 1), 0) for key, v in n.items()}


def split_numpy(p, sp, contigs, reads, wrong=None, ix=None):
    """every field of hs_map_segments, plus per read what the fork assertions read: detail[r] = a list of rounds, each with the number of free hits,
    the best key and score, the hits of the best per gap, the gap kept, n, the seed span (on the read as given) and whether the round ended the read"""
    assert split_valid(sp)
    k = p["k"]
    ix = mc.index_numpy(p, contigs) if ix is None else ix
    out = {f: [] for f in SEG_FIELDS}
    per = {f: np.zeros(len(reads), np.int64) for f in READ_FIELDS}
    seg_off, detail = [0], []
    for r, seq in enumerate(reads):
        Lr = len(seq)
        H = hits_numpy(p, ix, seq)
        per["n_minimizers"][r], per["n_skipped"][r], per["n_hits"][r] = H["n_minimizers"], H["n_skipped"], len(H["q"])
        q = H["q"]
        spans, segs, rounds = [], [], []
        for rnd in range(sp["max_segments"]):
            free = np.ones(len(q), bool)
            for a0, a1 in spans:
                free &= ((q + k - 1 <= a0) | (q + 1 >= a1)) if wrong == "overlap_one" else ((q + k <= a0) | (q >= a1))
            d = dict(n_free=int(free.sum()), taken=False)
            rounds.append(d)
            if not free.any():
                break
            score = _scores(H, free)
            cands = sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))
            if rnd == 0:
                best = cands[0][0]
                per["read_votes"][r] = cands[0][1]
                per["read_second"][r] = max([v for key, v in cands if key[:2] != best[:2] or abs(key[2] - best[2]) > 1] or [0])
            min_votes = p["min_votes"] if rnd == 0 or wrong == "index_min_votes" else sp["min_votes"]
            for best, votes in (cands if wrong == "skip" else cands[:1]):
                d.update(best=best, score=votes)
                if votes < min_votes:
                    break
                m = free & (H["c"] == best[0]) & (H["rel"] == best[1]) & ((H["b"] == best[2]) | (H["b"] == best[2] + 1))
                gap = np.zeros(len(q), np.int64)
                for a0, a1 in spans:
                    gap += a1 <= q
                counts = np.bincount(gap[m], minlength=len(spans) + 1)
                g = int(len(counts) - 1 - counts[::-1].argmax()) if wrong == "rightmost_gap" else int(counts.argmax())
                sel = m if wrong == "no_gap" else m & (gap == g)
                n = int(sel.sum())
                qa_lo, qa_hi, t_lo, t_hi = int(H["qa"][sel].min()), int(H["qa"][sel].max()) + k, int(H["t"][sel].min()), int(H["t"][sel].max()) + k
                a = (qa_lo, qa_hi) if best[1] == 0 else (Lr - qa_hi, Lr - qa_lo)
                d.update(gap_counts=counts.tolist(), gap=g, n=n, span=a)
                if rnd >= 1 and (n < min_votes or qa_hi - qa_lo < sp["min_span"]):
                    continue      # (the rule: `cands` has one entry, the rounds end; "skip": the next candidate)
                spans.append(a)
                segs.append(dict(key=best, n=n, second=per["read_second"][r] if rnd == 0 else 0, round=rnd, qa=(qa_lo, qa_hi), t=(t_lo, t_hi), a=a))
                d["taken"] = True
                break
            if not d["taken"]:
                break
        detail.append(rounds)
        segs.sort(key=lambda s: s["a"][0])
        for i, s in enumerate(segs):
            A0 = segs[i - 1]["a"][1] if i > 0 else 0
            A1 = segs[i + 1]["a"][0] if i + 1 < len(segs) else Lr
            if wrong != "always_extend":
                if i > 0 and s["a"][0] - segs[i - 1]["a"][1] > sp["max_gap"]:
                    A0 = s["a"][0]
                if i + 1 < len(segs) and segs[i + 1]["a"][0] - s["a"][1] > sp["max_gap"]:
                    A1 = s["a"][1]
            c, rel = s["key"][0], s["key"][1]
            (qa_lo, qa_hi), (t_lo, t_hi) = s["qa"], s["t"]
            if p["extend"]:
                b0, b1 = (A0, A1) if rel == 0 else (Lr - A1, Lr - A0)
                Lc = len(contigs[c])
                tl, th = t_lo - (qa_lo - b0), t_hi + (b1 - qa_hi)
                qa_lo, t_lo = b0 + max(0, -tl), max(0, tl)
                qa_hi, t_hi = b1 - max(0, th - Lc), min(Lc, th)
            qs, qe = (qa_lo, qa_hi) if rel == 0 else (Lr - qa_hi, Lr - qa_lo)
            for f, v in zip(SEG_FIELDS, (r, c, 1 - rel, qs, qe, t_lo, t_hi, s["n"], s["second"], s["round"])):
                out[f].append(v)
        seg_off.append(len(out["read"]))
    res = {f: np.array(out[f], np.int64) for f in SEG_FIELDS}
    res.update(per)
    res["seg_off"] = np.array(seg_off, np.int64)
    res["detail"] = detail
    return res


def n_wide(res):
    return int((res["n_hits"] > mc.LDS_CAPACITY).sum())


def rows(res, r=None):
    """the segments (of read r) as tuples (read, contig, strand, qstart, qend, tstart, tend)"""
    a, b = (0, len(res["read"])) if r is None else (int(res["seg_off"][r]), int(res["seg_off"][r + 1]))
    return [tuple(int(res[f][i]) for f in SEG_FIELDS[:7]) for i in range(a, b)]


def as_map_result(res):
    """a result with at most one segment per read in the shape of map_cases.map_numpy's (map_cases.FIELDS)"""
    n = len(res["seg_off"]) - 1
    assert (np.diff(res["seg_off"]) <= 1).all()
    out = {f: np.zeros(n, np.int64) for f in mc.FIELDS}
    out["contig"][:] = -1
    for f in ("n_minimizers", "n_hits", "n_skipped"):
        out[f] = np.asarray(res[f], np.int64)
    out["votes"], out["second"] = np.asarray(res["read_votes"], np.int64), np.asarray(res["read_second"], np.int64)
    m = np.asarray(res["read"], np.int64)
    for f in ("contig", "strand", "qstart", "qend", "tstart", "tend"):
        out[f][m] = res[f]
    return out


def paf(res, contigs, reads):
    lines = []
    for i in range(len(res["read"])):
        r, c = int(res["read"][i]), int(res["contig"][i])
        f = ["r%d" % r, len(reads[r]), res["qstart"][i], res["qend"][i], "+" if res["strand"][i] else "-", "c%d" % c, len(contigs[c]), res["tstart"][i], res["tend"][i],
             res["votes"][i], res["tend"][i] - res["tstart"][i], 255, "s1:i:%d" % res["votes"][i], "s2:i:%d" % res["second"][i], "sg:i:%d" % res["round"][i],
             "ns:i:%d" % (res["seg_off"][r + 1] - res["seg_off"][r])]
        lines.append("\t".join(str(x) for x in f) + "\n")
    return "".join(lines)


def same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in SEG_FIELDS + READ_FIELDS + ("seg_off",))


def differences(want, got):
    return [f for f in SEG_FIELDS + READ_FIELDS + ("seg_off",) if not np.array_equal(np.asarray(want[f], np.int64), np.asarray(got[f], np.int64))]


# ---- the selftest harness (tests/harness/map_split_selftest.cpp): the C++ host half of the rule ----
def run_harness(exe, p, sp, contigs, reads, threads=1):
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        f.write("%d %d %d %d %d %d %d %d\n" % (p["k"], p["w"], p["max_occ"], p["band_log2"], p["min_votes"], p["extend"], p["bucket_bits"], threads))
        f.write("%d %d %d %d\n" % (sp["max_segments"], sp["min_votes"], sp["min_span"], sp["max_gap"]))
        for seqs in (contigs, reads):
            f.write("%d\n" % len(seqs))
            for s in seqs:
                f.write(">" + "".join(map(str, np.asarray(s, np.uint8).tolist())) + "\n")
        f.flush()
        r = subprocess.run([exe, f.name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        return dict(returncode=r.returncode, stderr=r.stderr.decode())
    per = {f: np.zeros(len(reads), np.int64) for f in READ_FIELDS}
    n_segs = np.zeros(len(reads), np.int64)
    segs, text = [], []
    for line in r.stdout.decode().splitlines():
        t = line.split()
        if t[0] == "R":
            i = int(t[1])
            for f, v in zip(READ_FIELDS, t[2:7]):
                per[f][i] = int(v)
            n_segs[i] = int(t[7])
        elif t[0] == "S":
            segs.append([int(x) for x in t[2:]])
        else:
            text.append(line + "\n")
    a = np.array(segs, np.int64).reshape(-1, len(SEG_FIELDS))
    out = {f: a[:, i] for i, f in enumerate(SEG_FIELDS)}
    out.update(per)
    out["seg_off"] = np.concatenate([[0], np.cumsum(n_segs)]).astype(np.int64)
    out["text"] = "".join(text)
    out["returncode"] = 0
    return out


# ---- cases ----
def _rng(*seed):
    return np.random.default_rng([0x5350] + list(seed))


_rand = mc._rand


def parts_of(s, e, strand, cuts, total):
    """the parts of the read S[s:e] (strand 0: its reverse complement) on the pieces of S cut at `cuts`: (contig, strand, qstart, qend, tstart, tend)"""
    edges = [0] + list(cuts) + [total]
    out = []
    for c in range(len(edges) - 1):
        o0, o1 = max(s, edges[c]), min(e, edges[c + 1])
        if o0 < o1:
            qs, qe = (o0 - s, o1 - s) if strand else (e - o1, e - o0)
            out.append((c, strand, qs, qe, o0 - edges[c], o1 - edges[c]))
    return sorted(out, key=lambda x: x[2])


JUNCTION_CUTS = (10000, 20000, 21000)


def junction_reads(seed=77):
    """(whole sequence, [(start, end, strand)]): 6 reads over the cut at 10 000, 3 over 20 000 alone, 3 over 21 000 alone, 2 over both, and 30 anywhere
    -- each with 300 bases or more on every piece it reaches; 700 .. 4000 bases, both strands"""
    g = _rng(seed)
    S = _rand(g, 31000)
    spans = []
    for i in range(6):
        spans.append((10000 - int(g.integers(300, 2000)), 10000 + int(g.integers(400, 2000))))
    for i in range(3):
        spans.append((20000 - int(g.integers(400, 2000)), 20000 + int(g.integers(300, 900))))
    for i in range(3):
        spans.append((21000 - int(g.integers(300, 900)), 21000 + int(g.integers(400, 2000))))
    for i in range(2):
        spans.append((20000 - int(g.integers(300, 1400)), 21000 + int(g.integers(300, 1400))))
    while len(spans) < 44:      # (anywhere, but like the constructed ones with 300 bases or more on every piece they reach)
        L = int(g.integers(700, 4001))
        s = int(g.integers(0, 31000 - L + 1))
        if all(x[3] - x[2] >= 300 for x in parts_of(s, s + L, 1, JUNCTION_CUTS, 31000)):
            spans.append((s, s + L))
    return S, [(s, e, (i + int(g.integers(0, 2))) % 2 if i >= 14 else i % 2) for i, (s, e) in enumerate(spans)]


def _junction_exact():
    S, spans = junction_reads()
    edges = [0] + list(JUNCTION_CUTS) + [len(S)]
    contigs = [S[a:b] for a, b in zip(edges[:-1], edges[1:])]
    reads = [S[s:e] if st else rc(S[s:e]) for s, e, st in spans]
    return params(), split(), contigs, reads


def junction_truth():
    S, spans = junction_reads()
    return [[(i,) + x for x in parts_of(s, e, st, JUNCTION_CUTS, len(S))] for i, (s, e, st) in enumerate(spans)]


def _enclose():
    g = _rng(5)
    c0, c1 = _rand(g, 6000), _rand(g, 8000)
    read = np.concatenate([c0[1000:1600], c1[4000:6000], c0[3600:4200]])
    return params(), split(), [c0, c1], [read, rc(read)]


def _gap_tie():
    """the enclose read with as many hits of the shared key to the left of the middle part as to its right"""
    g = _rng(6)
    c0, c1 = _rand(g, 6000), _rand(g, 8000)
    p, sp = params(), split()
    ix = mc.index_numpy(p, [c0, c1])
    for L in range(500, 700):
        read = np.concatenate([c0[1000:1000 + L], c1[4000:6000], c0[3000 + L:3600 + L]])
        d = split_numpy(p, sp, [c0, c1], [read], ix=ix)["detail"][0]
        if len(d) > 1 and d[1].get("gap_counts") and d[1]["gap_counts"][0] == d[1]["gap_counts"][1]:
            return p, sp, [c0, c1], [read]
    raise AssertionError("no read with a tie between its gaps")


def _insert():
    """read 0: two parts of c0 around 1500 foreign bases; reads 1 and 2: c0 then c1 around a foreign stretch that leaves exactly max_gap | max_gap + 1
    bases between the two seed spans"""
    g = _rng(7)
    c0, c1, foreign = _rand(g, 5000), _rand(g, 5000), _rand(g, 1500)
    p, sp = params(), split()
    ix = mc.index_numpy(p, [c0, c1])
    reads = [np.concatenate([c0[1000:2000], foreign, c0[2000:3000]])]
    found = {}
    for off, F in ((off, F) for off in range(3000, 3040) for F in range(170, 215)):
        read = np.concatenate([c0[1000:2000], foreign[:F], c1[off:off + 1000]])
        res = split_numpy(p, sp, [c0, c1], [read], ix=ix)
        if len(res["read"]) != 2:
            continue
        a = sorted(d["span"] for d in res["detail"][0] if d["taken"])
        gap = a[1][0] - a[0][1]
        if gap in (sp["max_gap"], sp["max_gap"] + 1) and gap not in found:
            found[gap] = read
        if len(found) == 2:
            break
    assert len(found) == 2, "no foreign stretch that leaves exactly max_gap bases between the spans"
    return p, sp, [c0, c1], reads + [found[sp["max_gap"]], found[sp["max_gap"] + 1]]


def _three_parts():
    g = _rng(8)
    c = [_rand(g, 3000) for _ in range(3)]
    return params(), split(max_segments=2), c, [np.concatenate([c[0][500:1500], c[1][500:1300], c[2][500:1100]])]


def _nine_parts():
    g = _rng(9)
    c = [_rand(g, 400) for _ in range(9)]
    read = np.concatenate(c)
    return params(), split(max_segments=8), c, [read, rc(read)]


def _second_part_search(seed, sp, what, values, lengths):
    """reads c0[1000:1400] + c1[off:off + L] whose second part gives round 1 a candidate with `what` (score | seed span length) = each of `values`"""
    g = _rng(seed)
    c0, c1 = _rand(g, 3000), _rand(g, 3000)
    p = params()
    ix = mc.index_numpy(p, [c0, c1])
    found = {}
    for off in range(1000, 1400, 7):
        for L in lengths:
            read = np.concatenate([c0[1000:1400], c1[off:off + L]])
            d = split_numpy(p, sp, [c0, c1], [read], ix=ix)["detail"][0]
            if len(d) < 2 or "best" not in d[1] or d[1]["best"][0] != 1 or (what == "span" and "n" not in d[1]):
                continue
            v = d[1]["score"] if what == "score" else d[1]["span"][1] - d[1]["span"][0]
            if v in values and v not in found and (what == "score" or d[1]["n"] >= sp["min_votes"]):
                found[v] = read
        if len(found) == len(values):
            return p, sp, [c0, c1], [found[v] for v in values]
    raise AssertionError("no second part at the limit")


def _min_span():
    sp = split()
    return _second_part_search(10, sp, "span", (sp["min_span"] - 1, sp["min_span"]), range(95, 125))


def _min_votes():
    """split min_votes 5 above the index's 3: a second part of 4 | 5 hits, no bound on its span"""
    sp = split(min_votes=5, min_span=0)
    return _second_part_search(11, sp, "score", (sp["min_votes"] - 1, sp["min_votes"]), range(20, 70))


def _stop():
    """round 1's best candidate is a key with hits on both sides of the middle part; the side kept spans less than min_span = 300, and the rounds end
    although the part on c2 behind it spans more"""
    g = _rng(12)
    c = [_rand(g, 6000), _rand(g, 8000), _rand(g, 2000)]
    read = np.concatenate([c[0][1000:1250], c[1][4000:6000], c[0][3250:3500], c[2][100:500]])
    return params(), split(min_span=300), c, [read]


def _shared():
    """c1 holds a copy of the bases of c0 in front of the read's breakpoint: the k-mers there hit both contigs. extend = 0 and a search for a read in which
    a hit of round 1's candidate overlaps round 0's span by exactly one base"""
    p, sp = params(extend=0), split()
    for seed in range(40):
        g = _rng(13, seed)
        c0, c1 = _rand(g, 4000), _rand(g, 4000)
        n = int(g.integers(30, 80))
        c1[2000 - n:2000] = c0[2000 - n:2000]
        read = np.concatenate([c0[1000:2000], c1[2000:3200]])
        a = split_numpy(p, sp, [c0, c1], [read])
        if len(a["read"]) == 2 and not same(a, split_numpy(p, sp, [c0, c1], [read], wrong="overlap_one")):
            return p, sp, [c0, c1], [read, rc(read)]
    raise AssertionError("no read with a k-mer one base into a span")


def _wide(exact):
    """hits = LDS_CAPACITY (exact) | above it: a stretch of the 64-copy unit of map_cases' tandem construction, then 150 bases or more of another contig"""
    g = _rng(14)
    unit, uniq = _rand(g, 700), _rand(g, 3000)
    contigs = [np.tile(unit, 64), uniq]
    p, sp = params(), split()
    ix = mc.index_numpy(p, contigs)
    n_hits = lambda read: len(hits_numpy(p, ix, read)["q"])
    for la in range(420, 250, -1):
        make = lambda lb: np.concatenate([unit[:la], uniq[1000:1000 + lb]])
        if n_hits(make(150)) > mc.LDS_CAPACITY or n_hits(make(900)) < mc.LDS_CAPACITY + 1:
            continue
        lo, hi = 150, 900      # (a longer read has the shorter one's minimizers and more: the first length at or above the capacity)
        while lo < hi:
            mid = (lo + hi) // 2
            if n_hits(make(mid)) >= mc.LDS_CAPACITY:
                hi = mid
            else:
                lo = mid + 1
        if n_hits(make(lo)) != mc.LDS_CAPACITY:
            continue
        if exact:
            return p, sp, contigs, [make(lo)]
        while n_hits(make(lo)) == mc.LDS_CAPACITY:
            lo += 1
        return p, sp, contigs, [make(lo), rc(make(lo + 300))]
    raise AssertionError("no read with exactly the capacity's hits")


NOISY_CUT = 5000


@functools.lru_cache(maxsize=None)
def noisy():
    """test_cpu_map_cases.noisy_case() with its contig cut at 5 000: (the case, params, split params, contigs)"""
    from test_cpu_map_cases import noisy_case
    c = noisy_case()
    return c, params(), split(), [c.seq[:NOISY_CUT], c.seq[NOISY_CUT:]]


CASES = {
    "junction_exact": _junction_exact, "enclose": _enclose, "gap_tie": _gap_tie, "insert": _insert, "three_parts": _three_parts, "nine_parts": _nine_parts,
    "min_span": _min_span, "min_votes": _min_votes, "stop": _stop, "shared": _shared, "wide": lambda: _wide(False), "capacity": lambda: _wide(True),
}


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def want(name):
    """the numpy form's result of a case, computed once and shared"""
    p, sp, contigs, reads = get(name)
    return split_numpy(p, sp, contigs, reads)
