"""Seeded (query, target) pairs over byte alphabets for the tests of hs_edlib_align_bytes (tests/test_gpu_edlib_alphabets.py) and
the generator of their stored results (tests/golden/edlib_equalities_vectors.json.gz, stage5_bytes_cases.json; see README.md,
"Test vectors"). Only numpy's seeded Generator is used, so the same seed gives the same pairs; the stored files carry a digest
of the pairs they were made from. Sequences are uint8 arrays of the bytes themselves."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edlib_mode_pairs as P  # noqa: E402

SEED = 20261017
MODES = P.MODES
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# edlib's additionalEqualities of the two non-transitive relations the tests use: N matches every base (but A is not C), and
# the IUPAC ambiguity codes match the bases they stand for (and nothing else: R is not N, R is not M)
IUPAC = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
EQUALITIES = {
    "N": [("N", b) for b in "ACGT"],
    "IUPAC": [(c, b) for c, bases in IUPAC.items() for b in bases],
    "case": [(b.lower(), b) for b in "ACGT"],
}
AMBIGUOUS = {"N": np.frombuffer(b"N", dtype=np.uint8), "IUPAC": np.frombuffer("".join(IUPAC).encode(), dtype=np.uint8)}
AMBIGUITY_RATE = 0.05

GROUP_EDGES = (1, 63, 64, 65, 512, 513, 1024, 1025, 2048, 2049)      # query lengths at the boundaries of the lane groupings
BYTE_ALPHABETS = (5, 16, 17, 94, 256)                                  # LDS table: <= 16 symbols; scratch table above
BYTE_QUERY_LENGTHS = (1, 40, 63, 64, 65, 200, 513, 1030, 2100)


def equal_matrix(equalities):
    """256 x 256 bool: identity + the listed pairs, both ways (EqualityDefinition, edlib.cpp:61-92)"""
    m = np.eye(256, dtype=bool)
    for a, b in equalities:
        a, b = (x.encode()[0] if isinstance(x, str) else int(x) for x in (a, b))
        m[a, b] = m[b, a] = True
    return m


def _related(rng, q, kind, rate, max_len, mutate, random):
    """the target of query q: inside random flanks, a mutated copy, a truncated one, identical, unrelated"""
    if kind == 0:
        t = np.concatenate((random(int(rng.integers(0, 120))), mutate(q, rate), random(int(rng.integers(0, 120)))))
    elif kind == 1:
        t = mutate(q, rate)
    elif kind == 2:
        t = mutate(q, rate)[: max(1, int(len(q) * rng.uniform(0.1, 0.9)))]
    elif kind == 3:
        t = q.copy()
    else:
        t = random(P._length(rng, 1, max_len))
    t = t[:max_len]
    return t if len(t) else random(1)


def _sprinkle(rng, s, codes, rate):
    out = s.copy()
    hit = rng.random(len(s)) < rate
    out[hit] = rng.choice(codes, size=int(hit.sum()))
    return out


def eq_pairs(seed=SEED):
    """-> (pairs, kinds): ACGT pairs with about 5 % of the bases of both sequences replaced by N (kind "N") or by IUPAC ambiguity
    codes (kind "IUPAC"), in turn. 180 pairs of at most 400 x 400 (0-30 % edits; flanks, copies, truncated, identical, unrelated),
    one pair per kind at every query length of GROUP_EDGES, one of 4200 bases per kind (more than 64 blocks: two passes), and two
    that edlib cuts in halves (20 nb tn + 8 tn >= 1 MiB): 1500 x 2300 and 2300 x 1500."""
    rng = np.random.default_rng(seed)
    mutate = lambda s, rate: P._mutate(rng, s, rate)
    random = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    shapes = [(P._length(rng, 1, 400), 400, i % 5) for i in range(180)]
    shapes += [(qn, qn + 300, (0, 1)[j]) for qn in GROUP_EDGES for j in range(2)]
    shapes += [(4200, 4500, 0), (4200, 4500, 1)]
    pairs, kinds = [], []
    for i, (qn, max_len, kind) in enumerate(shapes):
        q = random(qn)
        t = _related(rng, q, kind, float(rng.uniform(0, 0.3)), max_len, mutate, random)
        pairs.append((q, t))
    q = random(1500)
    pairs.append((q, np.concatenate((random(400), mutate(q, 0.1), random(2300))).astype(np.uint8)[:2300]))
    q = random(2300)
    pairs.append((q, mutate(q, 0.15)[:1500]))
    out = []
    for i, (q, t) in enumerate(pairs):
        kind = ("N", "IUPAC")[i % 2]
        kinds.append(kind)
        out.append((_sprinkle(rng, ACGT[q], AMBIGUOUS[kind], AMBIGUITY_RATE), _sprinkle(rng, ACGT[t], AMBIGUOUS[kind], AMBIGUITY_RATE)))
    return out, kinds


def _mutate_sym(rng, s, rate, symbols):
    """as edlib_mode_pairs._mutate over any alphabet"""
    if rate <= 0 or len(s) == 0:
        return s.copy()
    u = rng.random(len(s))
    out = s.copy()
    sub = u < rate / 3
    out[sub] = rng.choice(symbols, size=int(sub.sum()))
    keep = ~((u >= rate / 3) & (u < 2 * rate / 3))
    ins = np.flatnonzero((u >= 2 * rate / 3) & (u < rate))
    out = np.insert(out, ins + 1, rng.choice(symbols, size=len(ins)))
    keep = np.insert(keep, ins + 1, True)
    return out[keep]


def byte_pairs(n_symbols, seed=SEED + 1):
    """pairs over n_symbols distinct bytes: printable ones (0x21-0x7e, no whitespace) up to 94, all of 0..255 for 256 (bytes 0 and
    255 are set in the longest pair). Two pairs at every query length of BYTE_QUERY_LENGTHS, one of 4200."""
    rng = np.random.default_rng(seed + n_symbols)
    symbols = np.arange(256, dtype=np.uint8) if n_symbols == 256 else rng.permutation(np.arange(0x21, 0x7f, dtype=np.uint8))[:n_symbols]
    mutate = lambda s, rate: _mutate_sym(rng, s, rate, symbols)
    random = lambda n: rng.choice(symbols, size=n)
    pairs = []
    for j, qn in enumerate(BYTE_QUERY_LENGTHS + BYTE_QUERY_LENGTHS + (4200,)):
        q = random(qn)
        pairs.append((q, _related(rng, q, j % 5, float(rng.choice([0.0, 0.05, 0.15, 0.3])), qn + 300, mutate, random)))
    q, t = pairs[-1]
    if n_symbols == 256:
        q[0] = 0; q[-1] = 255; t[1] = 255; t[-2] = 0
    return pairs


def case_pairs(seed=SEED + 2, n=150):
    """ACGT pairs of 1-1500 bases (edlib_mode_pairs.loc_pairs) with every base in lower case with probability 1/2"""
    rng = np.random.default_rng(seed)
    lower = lambda s: np.where(rng.random(len(s)) < 0.5, s | 0x20, s).astype(np.uint8)
    return [(lower(ACGT[q]), lower(ACGT[t])) for q, t in P.loc_pairs(seed, n, 1500)]


def upper(s):
    return (s & 0xDF).astype(np.uint8)


def renamed(pairs, seed=SEED + 3):
    """code arrays 0..3 under one random choice of four distinct bytes"""
    rng = np.random.default_rng(seed)
    names = rng.permutation(256)[:4].astype(np.uint8)
    return [(names[q], names[t]) for q, t in pairs]


digest = P.digest


def stage5_cases(seed=SEED + 4, n=42):
    """inputs of the two stage-5 call sites over ACGT + N runs, soft-masked lower case and IUPAC codes, n of each kind:
    reattach (tools.cpp:505-536): a backbone and a consensus that lost up to 60 bases at both ends; trim
    (create_new_contigs.cpp:556-629): a piece with overhangs and its polished copy"""
    rng = np.random.default_rng(seed)
    mutate = lambda s, rate: P._mutate(rng, s, rate)

    def dress(codes, style):
        s = ACGT[codes].copy()
        if style == 0:                                  # N runs next to ACGT
            for _ in range(int(rng.integers(1, 4))):
                a = int(rng.integers(0, len(s)))
                s[a:a + int(rng.integers(1, 30))] = ord("N")
        elif style == 1:                                # soft-masked stretches
            for _ in range(int(rng.integers(1, 4))):
                a = int(rng.integers(0, len(s)))
                b = a + int(rng.integers(10, 200))
                s[a:b] |= 0x20
        else:                                           # IUPAC codes from a polisher
            s = _sprinkle(rng, s, AMBIGUOUS["IUPAC"], 0.02)
        return s.tobytes().decode()

    cases = []
    for i in range(n):
        b = rng.integers(0, 4, size=int(rng.integers(250, 900)), dtype=np.uint8)
        c = mutate(b[int(rng.integers(0, 60)): len(b) - int(rng.integers(0, 60))], float(rng.uniform(0, 0.1)))
        cases.append({"kind": "reattach", "backbone": dress(b, i % 3), "consensus": dress(c, (i + i // 3) % 3)})
    for i in range(n):
        p = rng.integers(0, 4, size=int(rng.integers(350, 1000)), dtype=np.uint8)
        cases.append({"kind": "trim", "to_polish": dress(p, i % 3), "newcontig": dress(mutate(p, float(rng.uniform(0, 0.08))), (i + i // 3) % 3),
                      "overhang_left": int(rng.choice([0, 50, 150])), "overhang_right": int(rng.choice([0, 50, 150]))})
    return cases


def cases_digest(cases):
    import hashlib
    h = hashlib.sha256()
    for c in cases:
        for k in sorted(c):
            if k != "expected":
                h.update(("%s=%s;" % (k, c[k])).encode())
    return h.hexdigest()
