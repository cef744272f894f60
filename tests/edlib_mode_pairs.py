"""Seeded (query, target) pairs for the tests of hs_edlib_align (tests/test_gpu_edlib_modes.py) and the generator of their
stored results (tests/golden/edlib_modes_loc_vectors.json.gz, edlib_nw_shw_path_vectors.json.gz; see README.md, "Test
vectors"). Only numpy's seeded Generator is used, so the same seed gives the same pairs; the stored files carry a digest of
the pairs they were made from."""
import hashlib

import numpy as np

LOC_SEED = 20261016
LOC_PAIRS = 2000
MODES = ("NW", "SHW", "HW")
K_KINDS = ("-1", "0", "d-1", "d", "d+1")      # the bounds each pair is asked with: d = its distance with no bound


def _mutate(rng, s, rate):
    """substitutions, deletions and insertions, each at rate / 3 per base"""
    if rate <= 0 or len(s) == 0:
        return s.copy()
    u = rng.random(len(s))
    out = s.copy()
    sub = u < rate / 3
    out[sub] = (out[sub] + rng.integers(1, 4, size=int(sub.sum()), dtype=np.uint8)) & 3
    keep = ~((u >= rate / 3) & (u < 2 * rate / 3))
    ins = np.flatnonzero((u >= 2 * rate / 3) & (u < rate))
    out = np.insert(out, ins + 1, rng.integers(0, 4, size=len(ins), dtype=np.uint8))
    keep = np.insert(keep, ins + 1, True)
    return out[keep]


def _length(rng, lo, hi):
    """log-uniform in [lo, hi]"""
    return int(min(hi, max(lo, round(float(np.exp(rng.uniform(np.log(lo), np.log(hi))))))))


def loc_pairs(seed=LOC_SEED, n=LOC_PAIRS, max_len=3000):
    """n pairs of code arrays, lengths 1..max_len, 0-30 % edits. Kinds in turn: the query mutated inside random flanks, the query
    against a mutated copy of itself, a query longer than its target, identical pairs, unrelated pairs, tandem repeats."""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        kind = i % 6
        qn = _length(rng, 1, max_len)
        q = rng.integers(0, 4, size=qn, dtype=np.uint8)
        rate = float(rng.uniform(0, 0.3))
        if kind == 0:
            room = max_len - qn
            fl = [int(rng.integers(0, min(room, 400) + 1)) for _ in range(2)]
            t = np.concatenate((rng.integers(0, 4, size=fl[0], dtype=np.uint8), _mutate(rng, q, rate), rng.integers(0, 4, size=fl[1], dtype=np.uint8)))
        elif kind == 1:
            t = _mutate(rng, q, rate)
        elif kind == 2:
            t = _mutate(rng, q, rate)[: max(1, int(len(q) * rng.uniform(0.1, 0.9)))]
        elif kind == 3:
            t = q.copy()
        elif kind == 4:
            t = rng.integers(0, 4, size=_length(rng, 1, max_len), dtype=np.uint8)
        else:
            unit = rng.integers(0, 4, size=int(rng.integers(1, 7)), dtype=np.uint8)
            q = np.resize(unit, qn)
            t = np.concatenate((_mutate(rng, q, rate / 3), np.resize(unit, int(rng.integers(0, 20)))))
        t = t[:max_len]
        if len(t) == 0:
            t = rng.integers(0, 4, size=1, dtype=np.uint8)
        pairs.append((q, t.astype(np.uint8)))
    return pairs


def path_pairs(seed=LOC_SEED + 1):
    """pairs for the move-by-move comparison: every lane grouping of the path kernels (queries of <= 512, <= 1024, <= 2048
    bases whose matrix edlib keeps whole, longer ones on a wavefront each) and pairs of 20-24 kb that edlib cuts (Hirschberg)"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i, (lo, hi) in enumerate([(1, 64)] * 20 + [(65, 512)] * 40 + [(513, 1024)] * 25 + [(1025, 2048)] * 25 + [(2049, 6000)] * 10):
        qn = _length(rng, lo, hi)
        q = rng.integers(0, 4, size=qn, dtype=np.uint8)
        rate = float(rng.choice([0.0, 0.02, 0.08, 0.2, 0.3]))
        kind = i % 4
        if kind == 0:
            t = np.concatenate((rng.integers(0, 4, size=int(rng.integers(0, 200)), dtype=np.uint8), _mutate(rng, q, rate),
                                rng.integers(0, 4, size=int(rng.integers(0, 200)), dtype=np.uint8)))
        elif kind == 1:
            t = _mutate(rng, q, rate)
        elif kind == 2:
            t = _mutate(rng, q, rate)[: max(1, qn // 2)]
        else:
            t = rng.integers(0, 4, size=_length(rng, 1, 2 * qn + 1), dtype=np.uint8)
        pairs.append((q, t if len(t) else q[:1].copy()))
    for qn in (20000, 22000, 24000):
        q = rng.integers(0, 4, size=qn, dtype=np.uint8)
        pairs.append((q, _mutate(rng, q, 0.06)))
    return pairs


def digest(pairs):
    h = hashlib.sha256()
    for q, t in pairs:
        h.update(np.int64(len(q)).tobytes()); h.update(q.tobytes()); h.update(np.int64(len(t)).tobytes()); h.update(t.tobytes())
    return h.hexdigest()


def to_str(a):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[a].tobytes().decode()


def k_of(kind, d):
    """the bound of kind `kind` for a pair of distance d (None: the same as one already asked)"""
    if kind == "-1":
        return -1
    if kind == "0":
        return 0
    k = d + {"d-1": -1, "d": 0, "d+1": 1}[kind]
    return k if k > 0 else None
