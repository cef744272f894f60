"""Candidate columns for loop A of keep_only_robust_variants (call_variants.cpp:590-638), one builder per limit of the two forms the product has
(hs::cv_phase_a_host; k_loop_a_prepare -> k_loop_a -> k_loop_a_scan -> k_loop_a_pack), and a numpy restatement of the loop that also keeps the
books of the device form's documented limits (hs_kernels_loopa.hip, header comment). Only seeds and small parameters live here.

The domain, as the column selection guarantees it (call_variants.cpp:463-466): every column has at least 3 entries -- columns of 0 or 1 entries are
outside it and no case holds one --, positions ascend, the read indices of a column ascend, and every read of a column covers its position
(read_start <= pos < read_end): `Ctg.done()` asserts all of it. A case is a handful of contigs for ONE call; the two sides of a fork sit in sibling
contigs that differ in one column, so that the expected `failed` differs for exactly one reason.

| case     | what it sits on                                                                                                           |
| reads    | N = 2048 (a partition holds the read of rank 2047: word 31, bit 63), 2049 (33 words: not planned for the device), 64, 65  |
| words    | columns over 1, 2, 3, 4 words with entries at ranks 63|64, 127|128, ...; a 5-word column handed back; one skipped by `<= 5` |
| depth    | columns of 64, 65, 128 entries; 129 handed back                                                                           |
| codes    | 15 | 16 codes; reference code absent; reference code >= 128; tied second alleles: order bytes differ, equal, 7 keys      |
| slots    | 64 live partitions | a 65th | a 65th after one died by `pos >= reach` | by `right` 50 001 behind                         |
| pool     | partitions created = cap | cap + 1, cap = min(k + 8, k / div + 48)                                                       |
| ring     | hi_water - wlo = 8 (a read joins fresh in word w + 8 over a stale ring byte of word w) | 9                               |
| counters | more - less of one read = 255 | 256; fresh without a vote then a vote; opposing votes at 0 and 1; swapped < 0; nA == na    |
| rules    | pos - last_position 5|6 (last moves on augment only); |pos - right| 50 000|50 001; pos = reach - 1|reach; odd n / 2;        |
|          | 0.1 c / 0.9 c inexact in double (c = 10, 30, 70, 110); 2x2 tables around chi-square 15                                    |
| many     | 65 and 129 contigs in one call; contigs with 0 candidates, above the candidate bound, handed back in between             |

Not covered: numberOfOccurences >= 65535 (a 400-kb contig of augmenting columns), more than 1024 partitions of one contig in k_loop_a_pack, the repack
of collect_partitions when the span words do not fit (neither is reached by a case of a few seconds)."""
import numpy as np

from chi_tables import chi_square_reference, exact_tables, near_tables

FAR = 400_000            # default end of a read: beyond every position used here
A_, C_, G_, T_ = 65, 67, 71, 84
BOUND, DIV = 1 << 20, 6      # the candidate bound and pool divisor the tests pass unless a case says otherwise

_M1 = 0xc4ceb9fe1a85ec53
_MASK = (1 << 64) - 1


def order_byte(code):
    """hs::rh8_static_rank(code, false): the place of a byte key in the iteration order of the reference's hash map while it holds <= 6 keys"""
    h = code & 255
    h ^= h >> 33; h = (h * 0xff51afd7ed558ccd) & _MASK; h ^= h >> 33
    h = (h * _M1) & _MASK; h ^= h >> 33
    return int((((h >> 5) & 7) << 5) | (31 - (h & 31)))


class Ctg:
    """A contig under construction. Reads are addressed by RANK (start order); the read index of rank k is a seeded permutation, sorted inside groups
    of `group` equal starts, so that rank_of is not the identity and ties of the start position are broken by the index."""

    def __init__(self, n, seed, group=4):
        rng = np.random.default_rng(seed)
        perm = rng.permutation(n)
        for g in range(0, n, group):
            perm[g:g + group] = np.sort(perm[g:g + group])
        self.n = n
        self.read_of_rank = perm
        self.read_start = np.zeros(n, np.int64); self.read_start[perm] = np.arange(n) // group
        self.read_end = np.full(n, FAR, np.int64)
        self.pos, self.k0, self.cols = [], [], []

    def end(self, ranks, e):
        self.read_end[self.read_of_rank[np.asarray(ranks)]] = e

    def col(self, pos, k0, ranks, codes):
        r = self.read_of_rank[np.asarray(ranks, np.int64)]
        o = np.argsort(r)
        self.pos.append(pos); self.k0.append(k0); self.cols.append((r[o], np.asarray(codes, np.int64)[o]))

    def pair(self, pos, ranks, codes, k0=A_, gap=10):
        """a column and, `gap` behind it, the same column again (it fits what the first one left)"""
        self.col(pos, k0, ranks, codes); self.col(pos + gap, k0, ranks, codes)

    def done(self):
        S = len(self.pos)
        off = np.zeros(S + 1, np.int64)
        for k, (r, c) in enumerate(self.cols):
            off[k + 1] = off[k] + len(r)
            assert len(r) >= 3 and np.all(np.diff(r) > 0)
            assert np.all(self.read_start[r] <= self.pos[k]) and np.all(self.pos[k] < self.read_end[r]), "a read of a column does not cover its position"
        assert np.all(np.diff(self.pos) > 0)
        cat = lambda i, dt: np.concatenate([x[i] for x in self.cols]).astype(dt) if S else np.zeros(0, dt)
        return {"read_start": self.read_start.astype(np.int32), "read_end": self.read_end.astype(np.int32), "pos": np.array(self.pos, np.int32),
                "k0": np.array(self.k0, np.uint8), "off": off, "idx": cat(0, np.int32), "code": cat(1, np.uint8)}


def halves(n, a=A_, b=C_):
    return [a] * (n - n // 2) + [b] * (n // 2)


def rank_of(ctg):
    n = len(ctg["read_start"])
    order = np.lexsort((np.arange(n), ctg["read_start"]))
    rk = np.zeros(n, np.int64); rk[order] = np.arange(n)
    return rk


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------

def case_reads():
    out = []
    for N in (2048, 2049, 64, 65):
        c = Ctg(N, 100 + N)
        c.pair(1000, np.arange(0, 12), halves(12))
        c.pair(1020, np.arange(N - 12, N), halves(12))
        out.append(c.done())
    return {"contigs": out}


_WORD_SETS = {1: list(range(70, 82)), 2: list(range(250, 262)), 3: [445, 446, 447, 448, 449, 450, 509, 510, 511, 512, 513, 514],
              4: [702, 703, 704, 705, 766, 767, 768, 769, 830, 831, 832, 833],
              5: [766, 767, 768, 831, 832, 895, 896, 959, 960, 961, 962, 963], 14: list(range(900, 912))}


def case_words():
    out = []
    for kind in ("fits", "five_words", "five_words_skipped"):
        c = Ctg(1088, 7)
        for ww in (1, 2, 3, 4):
            c.pair(1000 + 100 * ww, _WORD_SETS[ww], halves(len(_WORD_SETS[ww])))
        if kind == "five_words":
            c.col(1500, A_, _WORD_SETS[5], halves(12))
        if kind == "five_words_skipped":
            c.col(1413, A_, _WORD_SETS[5], halves(12))      # 3 behind the column that augmented at 1410
        c.pair(1600, _WORD_SETS[14], halves(12, A_, G_))
        out.append(c.done())
    return {"contigs": out}


def case_depth():
    out = []
    for deep in (False, True):
        c = Ctg(192, 11)
        c.pair(1000, np.arange(0, 64), [A_, C_] * 32)
        c.pair(1100, np.arange(64, 129), ([A_, C_] * 33)[:65])
        c.pair(1200, np.arange(0, 128), [A_, A_, C_, C_] * 32)
        if deep:
            c.pair(1300, np.arange(0, 129), ([A_, A_, A_, C_] * 33)[:129])
        out.append(c.done())
    return {"contigs": out}


def _others(k, avoid):
    return [x for x in range(33, 127) if x not in avoid][:k]


def _tie_contig(seed, x, y, extra=()):
    """a partition over ranks 0..19 (ranks 0..9: +1, 10..19: -1), then a column whose shared reads carry the reference code 6 times (on +1 reads) and
    the codes x and y 4 times each: x on -1 reads, y on +1 reads. With x for the second allele the column fits, with y it does not. `extra`: more
    codes, one shared read each (more keys in the reference's hash map)."""
    c = Ctg(64, seed)
    c.pair(1000, np.arange(0, 20), [A_] * 10 + [C_] * 10)
    ranks = list(range(0, 6)) + list(range(6, 10)) + list(range(10, 14)) + [30]
    codes = [A_] * 6 + [y] * 4 + [x] * 4 + [x]      # (a fifth x outside the partition: a partition this column starts has no tie of its own)
    for k, e in enumerate(extra):
        ranks.append(14 + k); codes.append(e)
    c.col(1100, A_, ranks, codes)
    c.col(1200, A_, ranks, codes)
    return c.done()


def tie_pairs():
    """code pairs for the tie windows: (x, y) with different order bytes, and with the same one"""
    diff = [(x, y) for x in (C_, G_, T_, 45, 78) for y in (C_, G_, T_, 45, 78) if x != y and order_byte(x) != order_byte(y)]
    same = [(x, y) for x in range(40, 127) for y in range(40, 127) if x != y and A_ not in (x, y) and order_byte(x) == order_byte(y)]
    return diff[:8], same[:6]


def case_codes():
    out, kinds = [], []
    for n_other in (13, 14):      # 15 | 16 distinct codes
        c = Ctg(64, 21)
        oth = _others(n_other, (A_, C_))
        c.pair(1000, np.arange(0, 18 + n_other), [A_] * 10 + [C_] * 8 + oth)
        out.append(c.done()); kinds.append("codes%d" % (n_other + 2))
    c = Ctg(64, 22)      # the reference code is not in the column: ref_slot = -1, nA = 0
    c.pair(1000, np.arange(0, 14), [C_] * 8 + [G_] * 6, k0=90)
    out.append(c.done()); kinds.append("ref_absent")
    c = Ctg(64, 23)      # a reference code >= 128: the signed comparison of :838 leaves it eligible as the second allele
    c.pair(1000, np.arange(0, 14), [200] * 8 + [C_] * 6, k0=200)
    c.col(1100, 200, np.arange(0, 14), [200] * 5 + [C_] * 3 + [C_] * 3 + [G_] * 3)
    out.append(c.done()); kinds.append("ref_high")
    diff, same = tie_pairs()
    for k, (x, y) in enumerate(diff):
        out.append(_tie_contig(30 + k, x, y)); kinds.append("tie_fast")
    for k, (x, y) in enumerate(same):
        out.append(_tie_contig(50 + k, x, y)); kinds.append("tie_amb")
    for k, (x, y) in enumerate(diff[:4]):      # 7 keys: reference code, x, y and four more
        out.append(_tie_contig(70 + k, x, y, extra=_others(4, (A_, C_, x, y)))); kinds.append("tie_keys7")
    return {"contigs": out, "kinds": kinds}


def _slots_contig(n_parts, death=None):
    """64 partitions of 3 disjoint reads each (no shared read: neither fits nor correlates), then 41 columns that augment the first one -- the pool of
    k columns holds k / 6 + 48 partitions, 65 from k = 102 on --, then (n_parts = 65) a 65th. death: "reach" -- the reads of the partition on ranks
    3..5 end where the 65th column stands; "far" -- that partition was created 50 001 before it."""
    c = Ctg(256, 31)
    base = 60_000 if death == "far" else 1000
    pos65 = base + 7 * 64 + 7 * 41
    if death == "far":
        c.col(pos65 - 50_001, A_, [3, 4, 5], [A_, C_, C_])
    for p in range(64):
        if not (death == "far" and p == 1):
            c.col(base + 7 * p, A_, [3 * p, 3 * p + 1, 3 * p + 2], [A_, C_, C_])
    for k in range(41):
        c.col(base + 7 * 64 + 7 * k, A_, [0, 1, 2], [A_, C_, C_])
    if n_parts == 65:
        c.col(pos65, A_, [192, 193, 194], [A_, C_, C_])
    if death == "reach":
        c.end([3, 4, 5], pos65)
    return c.done()


def case_slots():
    return {"contigs": [_slots_contig(64), _slots_contig(65), _slots_contig(65, "reach"), _slots_contig(65, "far")]}


def pool_cap(k, div):
    return min(k + 8, k // div + 48)


def _pool_contig(k_cols, n_parts):
    """n_parts partitions on 3 disjoint reads each, every one dead (its reads end) before the next is created; the other columns augment partition 0"""
    c = Ctg(3 * n_parts + 3, 41)
    pos = 1000
    for p in range(1, n_parts):
        c.col(pos, A_, [3 * p, 3 * p + 1, 3 * p + 2], [A_, C_, C_])
        c.end([3 * p, 3 * p + 1, 3 * p + 2], pos + 1)
        pos += 7
    c.col(pos, A_, [0, 1, 2], [A_, C_, C_])
    for k in range(k_cols - n_parts):
        pos += 7
        c.col(pos, A_, [0, 1, 2], [A_, C_, C_])
    return c.done()


def case_pool(div=3):
    """k = 60 columns, divisor 3: cap = min(68, 20 + 48) = 68 -- more than k can create; so k = 60 with divisor 60: cap = min(68, 1 + 48) = 49"""
    k = 60
    cap = pool_cap(k, 60)
    return {"contigs": [_pool_contig(k, cap), _pool_contig(k, cap + 1)], "pool_div": 60, "k": k, "cap": cap}


def _ring_contig(last_word, late, again=False):
    """A partition starts in word 1 (ranks 64..75) and grows word by word: each column shares reads with it and brings fresh ones of a higher word
    (1 -> 4 -> 7 -> last_word). With last_word = 9 = 1 + 8 the fresh reads of ranks 576..578 join in the ring row of word 1, whose bytes for the same
    lanes (ranks 64..66) are stale and non-zero; `again` repeats that column (the byte a second vote reads must be the fresh one). late: a last column
    on reads of word 1, hi_water - wlo = last_word + 1 - 1."""
    c = Ctg(64 * 12, 51, group=2)
    c.pair(1000, np.arange(64, 76), halves(12))
    c.col(1100, A_, list(range(66, 74)) + list(range(256, 262)), [A_] * 4 + [C_] * 4 + [A_] * 3 + [C_] * 3)
    c.col(1110, A_, list(range(256, 262)) + list(range(448, 452)), [A_] * 3 + [C_] * 3 + [A_] * 2 + [C_] * 2)
    f = 64 * last_word
    for k in range(2 if again else 1):
        c.col(1120 + 10 * k, A_, list(range(448, 452)) + [f, f + 1, f + 2], [A_] * 2 + [C_] * 2 + [A_, C_, C_])
    if late:
        c.col(1200, A_, np.arange(64, 70), [A_] * 6)
    return c.done()


def case_ring():
    return {"contigs": [_ring_contig(8, True), _ring_contig(9, True), _ring_contig(9, False, again=True)]}


def _counter_contig(n_agree):
    """the read of rank 0 agrees n_agree times (created with more = 1, then n_agree - 1 columns six apart that augment)"""
    c = Ctg(64, 61)
    ranks = [0, 1, 2, 3, 4, 5]
    for k in range(n_agree):
        c.col(1000 + 6 * k, A_, ranks, [A_, A_, A_, C_, C_, C_])
    return c.done()


def _votes_contig():
    """vote sequences on one partition over ranks 0..11 (0..5: +1, 6..11: -1): a read fresh without a vote and then with one; an opposing vote at
    more - less = 0 (a state-0 read that voted once... then the state turns over) and at 1; a column whose phase vote is negative (swapped < 0);
    a column with nA == na"""
    c = Ctg(64, 62)
    c.col(1000, A_, np.arange(0, 12), [A_] * 6 + [C_] * 6)
    c.col(1010, A_, np.arange(0, 13), [A_] * 6 + [C_] * 6 + [G_])            # rank 12 joins fresh without a vote (state 0, more 0)
    c.col(1020, A_, np.arange(0, 13), [A_] * 6 + [C_] * 6 + [C_])            # ... and now votes: state -1, more 1 (1 - dold with dold = 0)
    c.col(1030, A_, np.arange(0, 13), [A_] * 6 + [C_] * 6 + [A_])            # opposing vote at more - less = 1: less += 1
    c.col(1040, A_, np.arange(0, 13), [A_] * 6 + [C_] * 6 + [A_])            # opposing vote at more - less = 0: the state turns over, more += 1
    c.col(1050, C_, np.arange(0, 12), [A_] * 6 + [C_] * 6)                   # reference code C: the phase vote is negative, the votes are swapped
    c.col(1060, A_, np.arange(0, 12), [A_] * 6 + [C_] * 6)                   # nA == na
    c.col(1070, A_, np.arange(0, 12), [A_] * 5 + [C_] * 7)                   # na > nA: 'a' is the most frequent character
    return c.done()


def case_counters():
    return {"contigs": [_counter_contig(255), _counter_contig(256), _votes_contig()]}


def _table_contig(seed, t, n_extra=0, k0=A_):
    """a partition over ranks 0..(A + B - 1) (+1 | -1), then one column with the 2x2 table t = (n00, n01, n10, n11) against it, plus n_extra reads
    outside the partition that carry the reference code"""
    n00, n01, n10, n11 = t
    a, b = n11 + n10, n01 + n00
    c = Ctg(max(a, 2) + max(b, 2) + n_extra + 4, seed)
    A, B = max(a, 2), max(b, 2)
    c.pair(1000, np.arange(0, A + B), [A_] * A + [C_] * B)
    ranks = list(range(0, a)) + list(range(A, A + b)) + list(range(A + B, A + B + n_extra))
    codes = [k0] * n11 + [G_] * n10 + [k0] * n01 + [G_] * n00 + [k0] * n_extra
    c.col(1100, k0, ranks, codes)
    c.col(1200, A_, np.arange(0, A + B), [A_] * A + [C_] * B)
    return c.done()


def rules_tables():
    """tables for the `rules` case: margins on both sides of 0.1 c and 0.9 c for c = 10, 30, 70, 110; n01 / n10 against max(0.1 s, 1.0); chi-square
    around 15 from tests/chi_tables.py, total <= 128 (a column of the device has at most 128 reads)"""
    tabs = []
    for c in (10, 30, 70, 110):
        lo = c // 10
        for s0 in (lo, lo + 1, c - lo, c - lo - 1):                      # n00 + n01 against 0.1 c and 0.9 c
            s1 = c - s0
            n01 = s0 // 2; n11 = max(lo + 1 - n01, min(s1, s1 // 2))
            if 0 <= n11 <= s1:
                tabs.append((s0 - n01, n01, s1 - n11, n11))
        for a2 in (lo, lo + 1, c - lo, c - lo - 1):                      # n01 + n11 against them
            n01 = a2 // 2; n11 = a2 - n01; s0 = c // 2
            if n01 <= s0 and n11 <= c - s0:
                tabs.append((s0 - n01, n01, c - s0 - n11, n11))
        s1 = min(c, 128 - c); lo1 = s1 // 10                                # (a column of the device holds at most 128 reads)
        for n01 in (lo - 1, lo, lo + 1):                                 # the fit's n01 <= max(0.1 (n00 + n01), 1.0) and n10 < max(0.1 (n11 + n10), 1.0)
            for n10 in (lo1 - 1, lo1, lo1 + 1):
                if n01 >= 0 and 0 <= n10 <= s1:
                    tabs.append((c - n01, n01, n10, s1 - n10))
    rng = np.random.default_rng(5)
    tabs += [t for t in exact_tables(15, 128)][:40]
    with np.errstate(divide="ignore", invalid="ignore"):      # (near_tables draws tables with an empty margin too, and drops them)
        tabs += [t for t in near_tables(15, 4000, rng, window=2.5, max_total=128) if min(t[0] + t[1], t[2] + t[3]) > 0][:160]
    return tabs


def float_estimate(t):
    """chi_square_gt15's single-precision estimate n (ad - bc)^2 / (r0 r1 c0 c1)"""
    f = np.float32
    n00, n01, n10, n11 = t
    r0, r1, c0, c1 = n00 + n01, n10 + n11, n00 + n10, n01 + n11
    if min(r0, r1, c0, c1) == 0:
        return None
    det = f(n00 * n11 - n01 * n10)
    return f(r0 + r1) * det * det / (f(r0) * f(r1) * f(c0) * f(c1))


def case_rules():
    out, kinds = [], []
    for gap in (5, 6):       # pos - last_position, where last_position moves on augment only
        c = Ctg(64, 71)
        c.pair(1000, np.arange(0, 12), halves(12))                       # created 1000, augmented 1010: last_position = 1010
        c.col(1010 + gap, A_, np.arange(20, 32), halves(12))             # 5: skipped; 6: creates
        c.col(1010 + gap + 3, A_, np.arange(20, 32), halves(12))         # 3 behind a column that only CREATED: not skipped when gap = 6 ... and
        c.col(1010 + gap + 12, A_, np.arange(20, 32), halves(12))        # ... 9 behind the one that augmented
        out.append(c.done()); kinds.append("gap%d" % gap)
    for far in (50_000, 50_001):
        c = Ctg(64, 72)
        c.pair(1000, np.arange(0, 12), halves(12))                       # right = 1010
        c.col(1010 + far, A_, np.arange(0, 12), halves(12))
        out.append(c.done()); kinds.append("far%d" % far)
    for d in (-1, 0):        # pos = reach - 1 | reach
        c = Ctg(64, 73)
        c.end(np.arange(0, 12), 1100)
        c.end([11], 1100 + (1 if d == -1 else 0))                        # reach - 1 = 1100: the read of rank 11 still covers it
        c.pair(1000, np.arange(0, 12), halves(12))
        c.col(1100, A_, ([11] if d == -1 else []) + list(range(20, 31)), ([C_] if d == -1 else []) + halves(11))
        out.append(c.done()); kinds.append("reach%d" % d)
    for n in (13, 15):       # comparable against n / 2 with odd n: 6 shared reads of 13 (13 / 2 = 6: enough), 6 of 15 (7: not enough)
        c = Ctg(64, 74)
        c.pair(1000, np.arange(0, 12), halves(12))
        c.col(1100, A_, [0, 1, 2, 6, 7, 8] + list(range(20, 20 + n - 6)), [A_] * 3 + [C_] * 3 + [A_] * (n - 6))
        out.append(c.done()); kinds.append("half%d" % n)
    tabs = rules_tables()
    for k, t in enumerate(tabs):
        out.append(_table_contig(1000 + k, t)); kinds.append("table")
    return {"contigs": out, "kinds": kinds, "tables": tabs}


def case_many(n_contigs):
    """n_contigs small contigs in one call: every 7th has no candidate, every 11th one column more than the bound (12), every 13th a 5-word column
    (handed back); the others two partitions each"""
    out, kinds = [], []
    for k in range(n_contigs):
        if k % 7 == 3:
            c = Ctg(16, 200 + k); out.append(c.done()); kinds.append("empty"); continue
        wide = k % 13 == 5
        c = Ctg(384 if wide else 40 + k % 30, 200 + k)
        n = 13 if k % 11 == 2 else 4 + k % 8
        for j in range(n // 2):
            c.pair(1000 + 40 * j, np.arange(3 * (j % 2), 3 * (j % 2) + 12), halves(12, A_, (C_, G_, T_)[(j + k) % 3]))
        if n % 2:
            c.col(1000 + 40 * (n // 2), A_, np.arange(20, 30), halves(10))
        if wide:
            c.col(3000, A_, [62, 63, 64, 127, 128, 191, 192, 255, 256, 257], halves(10))
        out.append(c.done()); kinds.append("above_bound" if n + (1 if wide else 0) > 12 else ("wide" if wide else "plain"))
    return {"contigs": out, "kinds": kinds, "bound": 12}


CASES = {"reads": case_reads, "words": case_words, "depth": case_depth, "codes": case_codes, "slots": case_slots, "pool": case_pool, "ring": case_ring,
         "counters": case_counters, "rules": case_rules, "many65": lambda: case_many(65), "many129": lambda: case_many(129)}
_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def to_i64(case):
    """the harness's `loop_a` input"""
    v = [np.array([len(case["contigs"])], np.int64)]
    for c in case["contigs"]:
        v.append(np.array([len(c["read_start"]), len(c["pos"]), len(c["idx"])], np.int64))
        for k in ("read_start", "read_end", "pos", "k0", "off", "idx", "code"):
            v.append(np.asarray(c[k]).astype(np.int64))
    return np.concatenate(v)


def from_i64(v, case):
    """the harness's `loop_a` output -> per contig {"rec": [P, 9], "state", "more", "less": [P, N]}"""
    out, at = [], 0
    for c in case["contigs"]:
        N = len(c["read_start"])
        P = int(v[at]); at += 1
        rec = np.zeros((P, 9), np.int64); st = np.zeros((P, N), np.int64); mo = np.zeros((P, N), np.int64); le = np.zeros((P, N), np.int64)
        for p in range(P):
            rec[p] = v[at:at + 9]; at += 9
            st[p] = v[at:at + N]; mo[p] = v[at + N:at + 2 * N]; le[p] = v[at + 2 * N:at + 3 * N]; at += 3 * N
        out.append({"rec": rec, "state": st, "more": mo, "less": le})
    assert at == len(v)
    return out


# ---- loop A restated, with the device form's limits on the side ---------------------------------------------------------------------------------

def tap_seconds(orc):
    c = orc["cmp"]
    return {(int(a), int(b)): int(s) for a, b, s, k in zip(c["col"], c["part"], c["second"], c["kind"]) if k == 1}


def restate(ctg, seconds, bound=BOUND, div=DIV, tie=None, last_on_create=False):
    """Loop A (:590-638) with Partition::Partition (Partition.cpp:32-83), distance (:778-967), computeChiSquare and augmentPartition (Partition.cpp:243-397)
    per read, in numpy. Second alleles: the most frequent code other than the reference code among the shared reads (the reference code itself stays
    eligible when it is >= 128, :838); of equal counts `tie` decides -- None: what the oracle's tap says for this (column, partition) (`seconds`),
    "lowest": the lowest code, "first": the one whose first read has the lowest index. last_on_create: the wrong form that moves last_position on
    create too. Alongside, the books of the device form (hs_kernels_loopa.hip): returns (partitions, fate, on_device, failed, reason) with
    partitions = {"rec": [P, 7] left, right, n_occ, n_corr, lo, hi, reach; "state", "more", "less": [P, N]}."""
    N, S = len(ctg["read_start"]), len(ctg["pos"])
    rk = rank_of(ctg)
    W = (N + 63) // 64
    on_device = 1 if 0 < S <= bound and W <= 32 else 0
    cap = pool_cap(S, div)
    parts, fate = [], []
    last, failed, reason, hi_water, n_ties = -5, 0, None, 0, 0

    def fail(why):
        nonlocal failed, reason
        if not failed:
            failed, reason = 1, why

    for ci in range(S):
        pos, k0 = int(ctg["pos"][ci]), int(ctg["k0"][ci])
        idx = ctg["idx"][ctg["off"][ci]:ctg["off"][ci + 1]].astype(np.int64); code = ctg["code"][ctg["off"][ci]:ctg["off"][ci + 1]].astype(np.int64)
        n = len(idx)
        if pos - last <= 5:
            fate.append((0, -1)); continue
        words = rk[idx] // 64
        wlo, ww = int(words.min()), int(words.max() - words.min() + 1)
        if n > 128 or ww > 4 or len(np.unique(code)) > 15:
            fail("column")
        hi_water = max(hi_water, wlo + ww)
        if hi_water - wlo > 8:
            fail("ring")
        live = [p for p in parts if p["live"] and abs(pos - p["right"]) <= 50000 and pos < p["reach"]]
        for p in parts:
            p["live"] = any(p is q for q in live)
        found, n_corr = None, 0
        for pi, p in enumerate(parts):
            if abs(pos - p["right"]) > 50000:
                continue
            st = p["state"][idx]
            sh = st != 2
            if not sh.any():
                continue
            cs, cnts = np.unique(code[sh], return_counts=True)
            elig = [(int(x), int(m)) for x, m in zip(cs, cnts) if x != k0 or k0 >= 128]
            second = 32
            if elig:
                best = max(m for _, m in elig)
                tied = [x for x, m in elig if m == best]
                if len(tied) == 1:
                    second = tied[0]
                else:
                    n_ties += 1
                    if tie is None:
                        second = seconds[(ci, pi)]
                    elif tie == "lowest":
                        second = min(tied)
                    else:
                        second = min(tied, key=lambda x: int(idx[sh & (code == x)].min()))
            isA = code == k0
            isa = (code == second) & ~isA
            n11 = int((isA & (st == 1)).sum()); n01 = int((isA & (st == -1)).sum()); n10 = int((isa & (st == 1)).sum()); n00 = int((isa & (st == -1)).sum())
            comparable = n00 + n01 + n10 + n11
            if (n00 + n01 > 0.1 * comparable and n00 + n01 < 0.9 * comparable and n01 + n11 > 0.1 * comparable and n01 + n11 < 0.9 * comparable
                    and chi_square_reference(n00, n01, n10, n11) > 15):
                n_corr += 1; p["n_corr"] += 1
            enough = comparable >= n // 2
            if ((n01 <= max(0.1 * (n00 + n01), 1.0) and n10 < max(0.1 * (n11 + n10), 1.0) and enough)
                    or (n00 <= max(0.1 * (n00 + n01), 1.0) and n11 < max(0.1 * (n11 + n10), 1.0) and enough)):
                found = pi
                nA, na = int(isA.sum()), int(isa.sum())
                if nA == 0 and na == 0:
                    vA = va = 0
                elif nA >= na:
                    vA, va = 1, (-1 if na > 0 else 0)
                else:
                    va, vA = 1, (-1 if nA > 0 else 0)
                v = np.where(isA, vA, np.where(isa, va, 0))
                if int((v * np.where(sh, st, 0)).sum()) < 0:
                    v = -v
                for r, s in zip(idx, v):
                    s = int(s); t = int(p["state"][r])
                    if t == 2:
                        p["state"][r] = s; p["more"][r] = abs(s); p["less"][r] = 0
                    elif s == 0:
                        pass
                    elif t == 0:
                        p["state"][r] = s; p["more"][r] = 1; p["less"][r] = 0
                    elif s == t:
                        p["more"][r] += 1
                    elif p["less"][r] + 1 > p["more"][r]:
                        p["state"][r] = -t; p["more"][r] += 1
                    else:
                        p["less"][r] += 1
                p["left"] = pos if (pos < p["left"] or p["left"] == -1) else p["left"]; p["right"] = max(p["right"], pos); p["n_occ"] += 1
                p["reach"] = max(p["reach"], int(ctg["read_end"][idx].max())); p["lo"] = min(p["lo"], int(idx.min())); p["hi"] = max(p["hi"], int(idx.max()))
                if int((p["more"][idx] - p["less"][idx]).max()) > 255 or p["n_occ"] >= 65535:
                    fail("counter")
                break
        if found is None:
            if len(parts) >= cap:
                fail("pool")
            elif sum(1 for p in parts if p["live"]) >= 64:
                fail("slots")
            cs, cnts = np.unique(code[code != k0], return_counts=True)
            assert len(cnts) == 0 or (cnts == cnts.max()).sum() == 1, "a tie for the second allele of a new partition: not restated"
            second = int(cs[np.argmax(cnts)]) if len(cnts) else -1
            st = np.full(N, 2, np.int64); st[idx] = np.where(code == k0, 1, np.where(code == second, -1, 0))
            mo = np.zeros(N, np.int64); mo[idx] = 1
            parts.append({"left": pos, "right": pos, "n_occ": 1, "n_corr": n_corr, "state": st, "more": mo, "less": np.zeros(N, np.int64), "live": True,
                          "reach": int(ctg["read_end"][idx].max()), "lo": int(idx.min()), "hi": int(idx.max())})
            fate.append((2, len(parts) - 1))
            if last_on_create:
                last = pos
        else:
            last = pos
            fate.append((1, found))
    P = len(parts)
    res = {"rec": np.array([[p[k] for k in ("left", "right", "n_occ", "n_corr", "lo", "hi", "reach")] for p in parts], np.int64).reshape(P, 7),
           "state": np.array([p["state"] for p in parts], np.int64).reshape(P, N), "more": np.array([p["more"] for p in parts], np.int64).reshape(P, N),
           "less": np.array([p["less"] for p in parts], np.int64).reshape(P, N), "n_ties": n_ties}
    return res, np.array(fate, np.int64).reshape(S, 2), on_device, (failed if on_device else 0), reason


_expected = {}


def expected(ol, name):
    """per contig of the case (oracle result, restatement, fate, on_device, failed, reason), computed once; ol = tests/oracle_lib"""
    if name not in _expected:
        case = get(name)
        out = []
        for c in case["contigs"]:
            o = ol.loop_a(len(c["read_start"]), c["pos"], c["k0"], c["off"], c["idx"], c["code"])
            out.append((o,) + restate(c, tap_seconds(o), case.get("bound", BOUND), case.get("pool_div", DIV)))
        _expected[name] = out
    return _expected[name]


def same_partitions(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ("state", "more", "less")) and np.array_equal(a["rec"][:, :4], b["rec"][:, :4])
