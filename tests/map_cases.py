"""The read mapper's rule (hairsplitter_amd/csrc/hs_map_host.h), restated in numpy, and the cases that reach its forks.

map_numpy(params, contigs, reads) is the rule with nothing shared with the C++ but the specification; `wrong` swaps one clause for a plausible
mistake, and tests/test_cpu_map_cases.py shows that the case named after the fork then gives another result. A case is (params, contigs, reads);
the two sides of a fork are sibling reads (or contigs) of one call. CASES lists them; get(name) builds one (cached)."""
import functools
import subprocess
import tempfile

import numpy as np

DEFAULT = dict(k=15, w=10, max_occ=64, band_log2=9, min_votes=3, extend=1, bucket_bits=-1)
LDS_CAPACITY = 4096      # hs_map_lds_capacity()
FIELDS = ("contig", "strand", "qstart", "qend", "tstart", "tend", "votes", "second", "n_minimizers", "n_hits", "n_skipped")
WRONG = ("rightmost", "palindromes", "one_bin", "qa_is_q", "tie_larger_contig", "second_adjacent", "occ_ge", "no_clip")
INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def rc(seq):
    return (3 - np.asarray(seq, np.uint8))[::-1].copy()


def mix32(x):
    """murmur3's 32-bit finaliser"""
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def kmers(seq, k, keep_palindromes=False):
    """hash, strand bit and validity of the k-mer at every position 0 .. L - k"""
    seq = np.asarray(seq, np.uint8)
    n = len(seq) - k + 1
    if n < 1:
        z = np.zeros(0, np.uint64)
        return z, z.astype(np.uint8), z.astype(bool)
    f = np.zeros(n, np.uint64); r = np.zeros(n, np.uint64)
    for i in range(k):
        c = (seq[i:i + n] & 3).astype(np.uint64)
        f |= c << np.uint64(2 * (k - 1 - i))
        r |= (np.uint64(3) - c) << np.uint64(2 * i)
    ok = (f != r) | keep_palindromes
    return mix32(np.minimum(f, r)), (r < f).astype(np.uint8), ok


def minimizers(seq, k, w, wrong=None):
    """(positions ascending, hashes, strand bits)"""
    h, s, ok = kmers(seq, k, keep_palindromes=wrong == "palindromes")
    n = len(h)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64), np.zeros(0, np.uint8)
    p = np.arange(n, dtype=np.uint64)
    tie = (np.uint64(0xFFFFFFFF) - p) if wrong == "rightmost" else p
    key = np.where(ok, (h << np.uint64(32)) | tie, INVALID)
    win = np.lib.stride_tricks.sliding_window_view(key, min(w, n))      # windows 0 .. max(0, n - w)
    arg = win.argmin(axis=1) + np.arange(len(win))
    arg = arg[win.min(axis=1) != INVALID]
    pos = np.unique(arg)
    return pos.astype(np.int64), h[pos], s[pos]


def index_numpy(p, contigs, wrong=None):
    hs, cs, ts, ss = [], [], [], []
    for c, seq in enumerate(contigs):
        pos, h, s = minimizers(seq, p["k"], p["w"], wrong)
        hs.append(h); cs.append(np.full(len(pos), c, np.int64)); ts.append(pos); ss.append(s)
    cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt)
    h, c, t, s = cat(hs, np.uint64), cat(cs, np.int64), cat(ts, np.int64), cat(ss, np.uint8)
    o = np.lexsort((t, c, h))
    n = len(h)
    bits = p["bucket_bits"]
    if bits < 0:
        bits = 10
        while bits < 26 and (1 << bits) < n:
            bits += 1
    return dict(h=h[o], c=c[o], t=t[o], s=s[o], bucket_bits=bits)


def index_entries(ix):
    """the index as sorted rows (bucket, hash, contig, t, strand bit): what any layout of the buckets must hold"""
    b = ix["h"] & np.uint64((1 << ix["bucket_bits"]) - 1)
    rows = np.stack([b.astype(np.int64), ix["h"].astype(np.int64), ix["c"], ix["t"], ix["s"].astype(np.int64)], axis=1) if len(b) else np.zeros((0, 5), np.int64)
    return rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))] if len(rows) else rows


def map_numpy(p, contigs, reads, wrong=None, ix=None):
    """every field of hs_map_result per read, plus what the fork assertions read: the read minimizers, the best key, the occ of looked-up and
    skipped minimizers, the hit count per bin of the best (contig, rel)"""
    k, band = p["k"], p["band_log2"]
    ix = index_numpy(p, contigs, wrong) if ix is None else ix      # (ix: the contigs' index, where a search calls this many times)
    out = {f: np.zeros(len(reads), np.int64) for f in FIELDS}
    out["contig"][:] = -1
    out["index"] = ix
    out["minimizers"] = []
    out["detail"] = []
    for r, seq in enumerate(reads):
        Lr = len(seq)
        pos, h, s = minimizers(seq, k, p["w"], wrong)
        out["minimizers"].append((pos, h, s))
        out["n_minimizers"][r] = len(pos)
        lo = np.searchsorted(ix["h"], h, "left"); hi = np.searchsorted(ix["h"], h, "right")
        occ = hi - lo
        skip = occ >= p["max_occ"] if wrong == "occ_ge" else occ > p["max_occ"]
        out["n_skipped"][r] = int(skip.sum())
        det = dict(occ_used=occ[~skip], occ_skipped=occ[skip], best=None, bins={})
        out["detail"].append(det)
        e = np.concatenate([np.arange(a, b) for a, b, sk in zip(lo, hi, skip) if not sk] or [np.zeros(0, np.int64)]).astype(np.int64)
        q = np.concatenate([np.full(b - a, x) for a, b, sk, x in zip(lo, hi, skip, pos) if not sk] or [np.zeros(0, np.int64)]).astype(np.int64)
        sq = np.concatenate([np.full(b - a, x) for a, b, sk, x in zip(lo, hi, skip, s) if not sk] or [np.zeros(0, np.int64)]).astype(np.int64)
        out["n_hits"][r] = len(e)
        if len(e) == 0:
            continue
        c, t = ix["c"][e], ix["t"][e]
        rel = sq ^ ix["s"][e].astype(np.int64)
        qa = q if wrong == "qa_is_q" else np.where(rel == 1, Lr - k - q, q)
        b = (t - qa + Lr) >> band
        hits = {}
        for key in zip(c.tolist(), rel.tolist(), b.tolist()):
            hits[key] = hits.get(key, 0) + 1
        score = {key: n + (0 if wrong == "one_bin" else hits.get((key[0], key[1], key[2] + 1), 0)) for key, n in hits.items()}
        order = (lambda kv: (-kv[1], -kv[0][0], kv[0][1], kv[0][2])) if wrong == "tie_larger_contig" else (lambda kv: (-kv[1], kv[0]))
        best, votes = min(score.items(), key=order)
        far = 0 if wrong == "second_adjacent" else 1
        second = max([v for key, v in score.items() if key[:2] != best[:2] or abs(key[2] - best[2]) > far] or [0])
        out["votes"][r], out["second"][r] = votes, second
        det["best"] = best
        det["bins"] = {key[2]: n for key, n in hits.items() if key[:2] == best[:2]}
        if votes < p["min_votes"]:
            continue
        m = (c == best[0]) & (rel == best[1]) & ((b == best[2]) | ((b == best[2] + 1) & (wrong != "one_bin")))
        qa_lo, qa_hi, t_lo, t_hi = int(qa[m].min()), int(qa[m].max()) + k, int(t[m].min()), int(t[m].max()) + k
        Lc = len(contigs[best[0]])
        if p["extend"]:
            tl, th = t_lo - qa_lo, t_hi + (Lr - qa_hi)
            if wrong == "no_clip":
                qa_lo, t_lo, qa_hi, t_hi = max(0, -tl), max(0, tl), Lr, th
            else:
                qa_lo, t_lo = max(0, -tl), max(0, tl)
                qa_hi, t_hi = Lr - max(0, th - Lc), min(Lc, th)
        out["contig"][r], out["strand"][r] = best[0], 1 - best[1]
        out["qstart"][r], out["qend"][r] = (qa_lo, qa_hi) if best[1] == 0 else (Lr - qa_hi, Lr - qa_lo)
        out["tstart"][r], out["tend"][r] = t_lo, t_hi
    return out


def n_wide(res):
    return int((res["n_hits"] > LDS_CAPACITY).sum())


def paf(res, contigs, reads):
    lines = []
    for i in range(len(reads)):
        c = int(res["contig"][i])
        if c < 0:
            continue
        f = [("r%d" % i), len(reads[i]), res["qstart"][i], res["qend"][i], "+" if res["strand"][i] else "-", "c%d" % c, len(contigs[c]), res["tstart"][i], res["tend"][i],
             res["votes"][i], res["tend"][i] - res["tstart"][i], 255, "s1:i:%d" % res["votes"][i], "s2:i:%d" % res["second"][i]]
        lines.append("\t".join(str(x) for x in f) + "\n")
    return "".join(lines)


def same(a, b):
    """do two results of map_numpy agree in everything a caller can see (fields, read minimizers, index)?"""
    if any(not np.array_equal(a[f], b[f]) for f in FIELDS):
        return False
    if any(not (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])) for x, y in zip(a["minimizers"], b["minimizers"])):
        return False
    return np.array_equal(index_entries(a["index"]), index_entries(b["index"]))


# ---- the selftest harness (tests/harness/map_selftest.cpp): the C++ host half of the rule ----
def write_job(path, p, contigs, reads, threads=1):
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d %d\n" % (p["k"], p["w"], p["max_occ"], p["band_log2"], p["min_votes"], p["extend"], p["bucket_bits"], threads))
        for seqs in (contigs, reads):
            f.write("%d\n" % len(seqs))
            for s in seqs:
                f.write(">" + "".join(map(str, np.asarray(s, np.uint8).tolist())) + "\n")


def run_harness(exe, p, contigs, reads, threads=1):
    """the harness's output in the shape of map_numpy's result (fields, minimizers, index rows, PAF text)"""
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        write_job(f.name, p, contigs, reads, threads)
        r = subprocess.run([exe, f.name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        return dict(returncode=r.returncode, stderr=r.stderr.decode())
    out = {f: np.zeros(len(reads), np.int64) for f in FIELDS}
    rows, mz, text = [], [[] for _ in reads], []
    bits = None
    for line in r.stdout.decode().splitlines():
        t = line.split()
        if t[0] == "INDEX":
            bits = int(t[1])
        elif t[0] == "E":
            rows.append([int(x) for x in t[1:]])
        elif t[0] == "M":
            mz[int(t[1])].append((int(t[2]), int(t[4]), int(t[3])))
        elif t[0] == "R":
            for f, v in zip(FIELDS, t[2:]):
                out[f][int(t[1])] = int(v)
        else:
            text.append(line + "\n")
    out["minimizers"] = [(np.array([x[0] for x in m], np.int64), np.array([x[1] for x in m], np.uint64), np.array([x[2] for x in m], np.uint8)) for m in mz]
    out["index_rows"] = np.array(rows, np.int64).reshape(-1, 5)
    out["bucket_bits"] = bits
    out["text"] = "".join(text)
    out["returncode"] = 0
    return out


def differences(want, got):
    """fields of `got` (the harness's or the device's) that differ from the numpy form's"""
    bad = [f for f in FIELDS if not np.array_equal(np.asarray(want[f], np.int64), np.asarray(got[f], np.int64))]
    if "minimizers" in got:
        for r, (x, y) in enumerate(zip(want["minimizers"], got["minimizers"])):
            if not (np.array_equal(x[0], y[0]) and np.array_equal(x[1].astype(np.uint64), y[1].astype(np.uint64)) and np.array_equal(x[2], y[2])):
                bad.append("minimizers of read %d" % r)
    if "index_rows" in got:
        rows = np.asarray(got["index_rows"], np.int64).reshape(-1, 5)
        rows = rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))] if len(rows) else rows
        if got["bucket_bits"] != want["index"]["bucket_bits"] or not np.array_equal(rows, index_entries(want["index"])):
            bad.append("index")
    return bad


# ---- cases ----
def _rng(*seed):
    return np.random.default_rng([0x4D41] + list(seed))


def _rand(rng, n):
    return rng.integers(0, 4, size=n).astype(np.uint8)


def _lengths():
    g = _rng(1)
    k, w = 15, 10
    c = _rand(g, 2000)
    reads = [c[100:100], c[100:100 + k - 1], c[200:200 + k], c[300:300 + k + w - 2], c[400:400 + k + w - 1], c[500:900]]
    return params(min_votes=1), [c, _rand(g, k - 1), _rand(g, 0)], reads


def _no_reads():
    return params(), [_rand(_rng(2), 500)], []


def _no_contig_minimizers():
    g = _rng(3)
    return params(), [_rand(g, 10), _rand(g, 0)], [_rand(g, 300), _rand(g, 5)]


def _no_contigs():
    return params(), [], [_rand(_rng(4), 200)]


def _kw(k, w):
    g = _rng(5, k, w)
    c = [_rand(g, 3000), _rand(g, 1500)]
    reads = [c[0][100:400], rc(c[0][1000:1300]), c[1][50:350], rc(c[1][1100:1500]), _rand(g, 300), c[0][2000:2000 + k + w - 1]]
    return params(k=k, w=w), c, reads


def _homopolymer():
    g = _rng(6)
    a, b, d = _rand(g, 300), _rand(g, 300), _rand(g, 300)
    run = np.zeros(100, np.uint8)
    di = np.tile(np.array([0, 1], np.uint8), 50)
    c = np.concatenate([a, run, b, di, d])
    return params(), [c], [c[250:450], rc(c[650:850]), c[320:380], c[720:780]]


def _palindromes():
    """k = 6: (AT)n holds palindromic 6-mers only; a window inside it names nothing"""
    g = _rng(7)
    at = np.tile(np.array([0, 3], np.uint8), 20)
    a, b = _rand(g, 200), _rand(g, 200)
    c = np.concatenate([a, at, b])
    return params(k=6, w=4, min_votes=1), [c], [c[150:300], at.copy(), rc(c[190:260])]


def _occ():
    """unit X 64 times and unit Y 65 times on the contig, each between spacers of its own; max_occ = 64"""
    g = _rng(8)
    x, y = _rand(g, 40), _rand(g, 40)
    parts = []
    for i in range(65):
        if i < 64:
            parts += [x, _rand(g, 40)]
        parts += [y, _rand(g, 40)]
    return params(min_votes=1), [np.concatenate(parts)], [x.copy(), y.copy()]


def _bins():
    g = _rng(9)
    c = _rand(g, 6000)
    Lr = 400
    edge = [c[1023 - Lr:1023], c[1024 - Lr:1024]]      # d + Lr = (2 << 9) - 1 | 2 << 9
    s = 1020 - 600
    indel = np.concatenate([c[s:s + 300], c[s + 310:s + 610]])      # a 10-base deletion moves the second half one bin up
    apart = np.concatenate([c[500:800], c[500 + 300 + 1536:500 + 600 + 1536]])      # the second half three bins up: must not add
    return params(), [c], edge + [indel, apart]


def _identical_contigs():
    g = _rng(10)
    c = _rand(g, 1500)
    return params(), [c, c.copy(), _rand(g, 1500)], [c[200:700], rc(c[800:1300])]


def _self_rc():
    g = _rng(11)
    x = _rand(g, 150)
    pal = np.concatenate([x, rc(x)])
    c = np.concatenate([_rand(g, 400), pal, _rand(g, 400)])
    return params(), [c], [pal.copy()]


def _ends(extend):
    g = _rng(12)
    c, small = _rand(g, 3000), _rand(g, 400)
    reads = []
    for h in (1, 200):
        reads += [np.concatenate([_rand(g, h), c[:500 - h]]), np.concatenate([c[3000 - 500 + h:], _rand(g, h)])]
        reads += [rc(reads[-2]), rc(reads[-1])]
    reads.append(np.concatenate([_rand(g, 100), small, _rand(g, 100)]))
    reads.append(rc(reads[-1]))
    return params(extend=extend), [c, small], reads


def _tandem():
    g = _rng(13)
    unit = _rand(g, 700)
    return params(), [np.tile(unit, 64), _rand(g, 1000)], [unit.copy(), rc(unit)]


def _capacity():
    """hits = LDS_CAPACITY | LDS_CAPACITY + 1: a stretch of the 64-copy unit plus bases of a unique contig, one base more or less"""
    g = _rng(14)
    unit, uniq = _rand(g, 700), _rand(g, 3000)
    contigs = [np.tile(unit, 64), uniq]
    p = params()
    ix = index_numpy(p, contigs)
    found = {}
    for la in range(420, 250, -1):
        found = {}
        for lb in range(40, 900):
            read = np.concatenate([unit[:la], uniq[1000:1000 + lb]])
            n = int(map_numpy(p, contigs, [read], ix=ix)["n_hits"][0])
            if n in (LDS_CAPACITY, LDS_CAPACITY + 1) and n not in found:
                found[n] = read
            if n > LDS_CAPACITY + 1:
                break
        if len(found) == 2:
            break
    assert len(found) == 2, "no read with exactly the capacity's hits"
    return p, contigs, [found[LDS_CAPACITY], found[LDS_CAPACITY + 1]]


def _buckets(bits):
    p, c, r = _kw(15, 10)
    return params(bucket_bits=bits), c, r


def _unmapped():
    """a random read; a read whose best score is min_votes - 1 | min_votes"""
    g = _rng(15)
    c = _rand(g, 2000)
    p = params()
    found = {}
    for n in range(24, 200):
        read = c[700:700 + n]
        v = int(map_numpy(p, [c], [read])["votes"][0])
        if v in (p["min_votes"] - 1, p["min_votes"]) and v not in found:
            found[v] = read
    assert len(found) == 2
    return p, [c], [_rand(g, 500), found[p["min_votes"] - 1], found[p["min_votes"]]]


def exact_reads(seed=16, length=20000, n=60):
    """error-free reads of a random contig, both strands, k + w - 1 bases and more: (params, contig, reads, starts, strands)"""
    g = _rng(seed)
    c = _rand(g, length)
    p = params(min_votes=1)
    lens = [p["k"] + p["w"] - 1, p["k"] + p["w"], 100, 511, 512, 513] + [int(x) for x in g.integers(24, 3000, size=n - 6)]
    starts = [0, length - lens[1]] + [int(g.integers(0, length - L + 1)) for L in lens[2:]]
    strands = [int(x) for x in g.integers(0, 2, size=n)]
    reads = [c[s:s + L] if st else rc(c[s:s + L]) for s, L, st in zip(starts, lens, strands)]
    return p, c, reads, starts, strands


def _exact():
    p, c, reads, _, _ = exact_reads()
    return p, [c], reads


CASES = {
    "lengths": _lengths, "no_reads": _no_reads, "no_contig_minimizers": _no_contig_minimizers, "no_contigs": _no_contigs,
    "k5_w1": lambda: _kw(5, 1), "k5_w32": lambda: _kw(5, 32), "k15_w10": lambda: _kw(15, 10), "k16_w1": lambda: _kw(16, 1), "k16_w32": lambda: _kw(16, 32),
    "homopolymer": _homopolymer, "palindromes": _palindromes, "occ": _occ, "bins": _bins, "identical_contigs": _identical_contigs, "self_rc": _self_rc,
    "ends_extend0": lambda: _ends(0), "ends_extend1": lambda: _ends(1), "tandem": _tandem, "capacity": _capacity,
    "buckets_one": lambda: _buckets(0), "buckets_eight": lambda: _buckets(3), "unmapped": _unmapped, "exact": _exact,
}


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def want(name):
    """the numpy form's result of a case, computed once and shared"""
    p, contigs, reads = get(name)
    return map_numpy(p, contigs, reads)
