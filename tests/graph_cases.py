"""Stage-4 inputs (hs_sr_contig: reads, SNP columns) built directly, without stage 3, at the shapes where the front of stage 4 -- K5a k_snp_planes, K5
k_simdiff, k_simdiff_windows, K6 k_read_graph_rows<LM> and the row fetch / patch / degree / fill kernels -- takes another path, in the layout hs_sr_run
launches them in. Used by tests/test_cpu_graph_cases.py (which proves, with the oracle and numpy alone, that every case is what it claims to be) and
tests/test_gpu_graph_front.py.

A case is {"contigs": [contig dict ...], "window": w, "error_rate": e, "low_memory": bool}. A contig dict holds what hairsplitter_amd.api takes (length,
read_start, read_end, snp_pos, snp_ref, snp_alt, col_off, col_idx, col_code) plus "mask_sizes": the number of reads of each of its graph windows, as designed, and "hap": the haplotype every read was drawn from.

Every SNP column lists every read that covers the position (ascending read index), except where a case says otherwise. A read carries the reference or the
alternative allele of its haplotype, flipped with probability `noise`, or -- with probability `third` -- a third allele that counts for neither plane.

Shapes of the windows: one window of 2000 positions with SNPs on a contig of 2150 unless stated (the contig's second window, [2000, 2151), has none). The SNPs sit in two clumps at 500.. and 1900.. (each within ten
positions, so that the oracle's whole-contig run seeds few Chinese-Whispers runs): the window's mask is the reads present at the first AND the last SNP, so
reads that end at 1200 or start at 1201 are in the columns but not in the mask. Reads start at 0 .. 39, unrelated to their index."""
import numpy as np

WINDOW = 2000
LENGTH = 2150
BASES = np.frombuffer(b"ACGT", np.uint8)


def _columns(rng, read_start, read_end, snp_pos, hap, n_hap=3, noise=0.02, third=0.03, pattern=None):
    """-> snp_ref, snp_alt, col_off, col_idx, col_code (and the third allele of every SNP) for reads with haplotypes `hap`
    (pattern: a function (rng, S, n_hap) -> the allele of every haplotype at every SNP, instead of independent draws)"""
    N, S = len(read_start), len(snp_pos)
    pick = np.argsort(rng.random((S, 4)), axis=1)[:, :3]      # three different bases per SNP
    snp_ref, snp_alt, snp_third = BASES[pick[:, 0]], BASES[pick[:, 1]], BASES[pick[:, 2]]
    pattern = rng.integers(0, 2, (S, n_hap)) if pattern is None else pattern(rng, S, n_hap)      # allele of every haplotype at every SNP (1 = alternative)
    off, idx, code = [0], [], []
    for s in range(S):
        r = np.nonzero((read_start <= snp_pos[s]) & (read_end >= snp_pos[s]))[0].astype(np.int32)
        a = pattern[s, hap[r]] ^ (rng.random(len(r)) < noise)
        c = np.where(a == 1, snp_alt[s], snp_ref[s]).astype(np.uint8)
        c[rng.random(len(r)) < third] = snp_third[s]
        idx.append(r); code.append(c); off.append(off[-1] + len(r))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return snp_ref.copy(), snp_alt.copy(), np.array(off, np.int64), cat(idx, np.int32), cat(code, np.uint8), snp_third


def _contig(rng, length, read_start, read_end, snp_pos, mask_sizes, **kw):
    read_start = np.asarray(read_start, np.int32); read_end = np.asarray(read_end, np.int32); snp_pos = np.asarray(snp_pos, np.int32)
    n_hap = kw.get("n_hap", 3)
    hap = kw.pop("hap", None)      # (given: the haplotype of every read; else drawn)
    if hap is None:
        hap = rng.integers(0, n_hap, len(read_start))
    ref, alt, off, idx, code, third = _columns(rng, read_start, read_end, snp_pos, hap, **kw)
    return {"length": int(length), "read_start": read_start, "read_end": read_end, "snp_pos": snp_pos, "snp_ref": ref, "snp_alt": alt, "col_off": off,
            "col_idx": idx, "col_code": code, "snp_third": third, "mask_sizes": list(mask_sizes), "hap": np.asarray(hap)}


def clump_positions(S):
    """S positions, ascending: the first half within [500, 510), the second within [1900, 1910)"""
    h = (S + 1) // 2
    a = 500 + (np.arange(h) * 10) // max(h, 1)
    b = 1900 + (np.arange(S - h) * 10) // max(S - h, 1)
    return np.concatenate((a, b)).astype(np.int32)


def one_window_contig(rng, N, m, S, snp_pos=None, balanced=False, full_ids=None, length=None, **kw):
    """N reads, S SNPs, one window whose mask holds m of the reads: those span the contig, the others end at 1200 or start at 1201 by turns (they are in
    the columns of one clump only). S == 1: first and last SNP are the same column, the mask is everything that covers it.
    snp_pos: the S positions instead of the two clumps (the first at 1200 or before, the last behind 1200, for the mask to be the m reads).
    balanced: the m reads are dealt to the n_hap haplotypes in turn (equal sizes up to one), the others drawn.
    full_ids: the m reads themselves (the highest index among them) instead of a draw. length: of the contig, where it is longer than the reads reach
    (windows behind the first hold no SNP; the coverage falls)."""
    full = np.zeros(N, bool)
    if full_ids is not None:
        assert len(full_ids) == m and max(full_ids) == N - 1
        full[np.asarray(full_ids)] = True
    elif m > 0:
        chosen = rng.permutation(N - 1)[:m - 1] if N > 1 else np.zeros(0, np.int64)
        full[chosen] = True; full[N - 1] = True      # (the read with the highest index is in the last column: see the reference's mask loop)
    start = rng.integers(0, 40, N).astype(np.int32); end = np.full(N, LENGTH - 1, np.int32)      # (start order != read order: the matrices' rows are permuted)
    is_left = (N - 1 - np.arange(N)) % 2 == 1      # (by turns, and the highest index on the right: in the last column)
    end[~full & is_left] = 1200
    start[~full & ~is_left] = 1201
    if S == 1 and snp_pos is None:
        m = int(np.sum(start <= 500))
    if balanced:
        n_hap = kw.get("n_hap", 3)
        hap = rng.integers(0, n_hap, N)
        who = np.flatnonzero(full)
        hap[who[rng.permutation(len(who))]] = np.arange(len(who)) % n_hap
        kw["hap"] = hap
    return _contig(rng, LENGTH if length is None else length, start, end, clump_positions(S) if snp_pos is None else snp_pos, [m] if S > 0 else [], **kw)


# ---- the cases ----
def case_blocks():
    rng = np.random.default_rng(101)
    shapes = [(1, 64), (2, 1), (63, 65), (64, 255), (65, 256), (511, 257), (512, 1), (513, 64), (600, 1025), (64, 1025), (65, 1)]
    return {"contigs": [one_window_contig(rng, N, N, S) for N, S in shapes], "window": WINDOW, "error_rate": 0.05, "low_memory": False}


def case_packed(low_memory=False, seed=102, sizes=((40, 40, 70), (30, 30, 0), (50, 44, 256), (20, 20, 3), (45, 37, 130))):
    rng = np.random.default_rng(seed)
    return {"contigs": [one_window_contig(rng, N, m, S) for N, m, S in sizes], "window": WINDOW, "error_rate": 0.05, "low_memory": low_memory}


def _tiled_reads(rng, n_tiles, n_lone, n_dead, length):
    """reads of 2500 to 3500 positions on a grid of 250 starts (many equal starts); n_lone reads of one position between two SNPs and a block of n_dead
    reads in front of the first SNP (none of them in any column); the read index is a random permutation of the start order"""
    start = 250 * rng.integers(1, (length - 2600) // 250, n_tiles)
    end = np.minimum(start + rng.integers(2500, 3500, n_tiles), length - 1)
    lone = 301 + 4 * rng.integers(0, 2000, n_lone)      # (SNPs at 300 + 4 s)
    start = np.concatenate((np.zeros(n_dead, np.int64), start, lone)); end = np.concatenate((np.full(n_dead, 40), end, lone))
    p = rng.permutation(len(start))
    return start[p].astype(np.int32), end[p].astype(np.int32)


def case_tiled():
    rng = np.random.default_rng(103)
    S, length = 2100, 8900      # 33 words; windows [0, 2000) .. [6000, 8000), [8000, 8901)
    snp_pos = 300 + 4 * np.arange(S)
    start, end = _tiled_reads(rng, 320, 16, 64, length)      # N = 400; the 64 reads at 0..40 are the first 64-row block of the matrices
    c = _contig(rng, length, start, end, snp_pos, [], noise=0.02, third=0.03)
    c["mask_sizes"] = None      # (not designed: whatever spans a window)
    return {"contigs": [c], "window": WINDOW, "error_rate": 0.05, "low_memory": False}


def case_fringe():
    """Blocks of 64 reads (in start order) whose presence ends in word 15, 16, 17 or begins in word 15, 16, 17, and 16 reads behind them. The first and
    the last SNP every read is present at carry a third allele only: the range of a read comes from presence, not from its plane bits."""
    rng = np.random.default_rng(104)
    S, length = 2100, 8900
    snp_pos = 300 + 4 * np.arange(S)
    at = lambda s: 300 + 4 * s
    groups = [(300, at(16 * 64 - 1)), (301, at(17 * 64 - 1)), (302, at(18 * 64 - 1)), (at(15 * 64), length - 1), (at(16 * 64), length - 1), (at(17 * 64), length - 1)]
    start = np.concatenate([np.full(64, a) for a, _ in groups] + [np.full(16, at(17 * 64 + 1))])      # (the last 16 rank behind the six blocks)
    end = np.concatenate([np.full(64, b) for _, b in groups] + [np.full(16, length - 1)])
    p = rng.permutation(len(start))
    inv = np.argsort(p)
    start, end = start[p].astype(np.int32), end[p].astype(np.int32)
    c = _contig(rng, length, start, end, snp_pos, [], noise=0.02, third=0.03)
    # the first and the last entry of every read: third allele
    seg = np.repeat(np.arange(S), np.diff(c["col_off"]))
    E = len(seg)
    first = np.unique(c["col_idx"], return_index=True)[1]
    last = E - 1 - np.unique(c["col_idx"][::-1], return_index=True)[1]
    for e in (first, last):
        c["col_code"][e] = c["snp_third"][seg[e]]
    c["mask_sizes"] = None
    c["groups"] = [inv[64 * g:64 * (g + 1)] for g in range(6)]      # read indices of the six blocks
    return {"contigs": [c], "window": WINDOW, "error_rate": 0.05, "low_memory": False}


def case_ties():
    rng = np.random.default_rng(105)
    return {"contigs": [one_window_contig(rng, 150, 150, 16, n_hap=2, noise=0.15, third=0.0) for _ in range(8)], "window": WINDOW, "error_rate": 0.05,
            "low_memory": False}


def case_small_m():
    rng = np.random.default_rng(106)
    shapes = [(9, 0, 8), (9, 1, 8), (1, 1, 3), (10, 2, 8), (12, 5, 8), (12, 6, 8), (80, 64, 8), (80, 65, 8)]
    cs = [one_window_contig(rng, N, m, S) for N, m, S in shapes]
    return {"contigs": cs, "window": WINDOW, "error_rate": 0.05, "low_memory": False}


def case_wide():
    """1800 reads over the window [2000, 4000) of a contig of 6200 (coverage 1800 x 2101 / 6200 = 610) and 24 short ones beside it"""
    rng = np.random.default_rng(107)
    N, length = 1824, 6200
    start = np.full(N, 1950, np.int32); end = np.full(N, 4050, np.int32)
    short = rng.permutation(N - 1)[:24]
    start[short] = 3000      # in the second clump only
    snp_pos = np.concatenate((2010 + np.arange(12) // 2, 3900 + np.arange(12) // 2))
    c = _contig(rng, length, start, end, snp_pos, [1800], noise=0.03, third=0.03)
    return {"contigs": [c], "window": WINDOW, "error_rate": 0.05, "low_memory": False}


def case_lm_flag():
    return case_packed(True, 108, ((70, 63, 70), (30, 30, 0), (70, 64, 256), (70, 65, 3), (140, 130, 130)))


def case_lm_mixed():
    rng = np.random.default_rng(109)
    cs = [one_window_contig(rng, 50, 44, 70), one_window_contig(rng, 1040, 1040, 20), one_window_contig(rng, 45, 37, 130)]
    return {"contigs": cs, "window": WINDOW, "error_rate": 0.05, "low_memory": False}


def case_lm_nan():
    rng = np.random.default_rng(110)
    cs = [one_window_contig(rng, 40, 36, 3, third=0.45), one_window_contig(rng, 70, 66, 2, third=0.5)]
    return {"contigs": cs, "window": WINDOW, "error_rate": 0.05, "low_memory": True}


def case_lm_gap():
    """two low-memory contigs; in the second, one read of the mask is missing from a SNP column between its first and its last one"""
    rng = np.random.default_rng(111)
    cs = [one_window_contig(rng, 40, 36, 6), one_window_contig(rng, 40, 36, 6)]
    c = cs[1]
    s = 2
    col = lambda k: c["col_idx"][c["col_off"][k]:c["col_off"][k + 1]]
    r = int(np.intersect1d(np.intersect1d(col(0), col(s)), col(5))[0])      # a read of the mask (present at the first and the last SNP)
    e = int(c["col_off"][s]) + int(np.nonzero(col(s) == r)[0][0])
    c["gap"] = (r, s)
    c["col_idx"] = np.delete(c["col_idx"], e); c["col_code"] = np.delete(c["col_code"], e)
    c["col_off"] = c["col_off"].copy(); c["col_off"][s + 1:] -= 1
    return {"contigs": cs, "window": WINDOW, "error_rate": 0.05, "low_memory": True}


CASES = {"blocks": case_blocks, "packed": case_packed, "tiled": case_tiled, "fringe": case_fringe, "ties": case_ties, "small_m": case_small_m, "wide": case_wide,
         "lm_flag": case_lm_flag, "lm_mixed": case_lm_mixed, "lm_nan": case_lm_nan, "lm_gap": case_lm_gap}
_made = {}


def register(name, case):
    """a case made elsewhere (stage-4 inputs that stage 3 produced), under a name of its own"""
    assert name not in CASES and name not in _made
    _made[name] = case


def get(name):
    """the case, built once per process (read-only: copy before changing anything)"""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


# ---- plain restatements of the rules the cases are built around ----
def coverage_above_1000(c):
    """separate_reads.cpp:1515-1518: float accumulation of the read lengths, over the contig length"""
    cov = np.float32(0)
    for a, b in zip(c["read_start"], c["read_end"]):
        cov = np.float32(cov + np.float32(int(b) - int(a) + 1))
    return bool(np.float32(cov / np.float32(c["length"])) > 1000)


def expected_planes(c):
    """alt / ref bit rows [N, words] of a contig: bit (r, s) = code == alt / code == ref"""
    N, S = len(c["read_start"]), len(c["snp_pos"])
    W = (S + 63) // 64
    alt = np.zeros((N, max(W, 1)), np.uint64); ref = np.zeros((N, max(W, 1)), np.uint64)
    seg = np.repeat(np.arange(S), np.diff(c["col_off"]))
    bit = np.left_shift(np.uint64(1), (seg % 64).astype(np.uint64))
    for plane, allele in ((alt, c["snp_alt"]), (ref, c["snp_ref"])):
        hit = c["col_code"] == allele[seg]
        if plane is alt:
            hit &= c["col_code"] != c["snp_ref"][seg]      # (ref is tested first: the planes are disjoint)
        np.bitwise_or.at(plane, (c["col_idx"][hit], seg[hit] // 64), bit[hit])
    return alt[:, :W], ref[:, :W]


def presence_words(c):
    """first and last 64-SNP word every read is present in (any code); (big, -1) for a read in no column"""
    N = len(c["read_start"])
    lo = np.full(N, 2 ** 31 - 1, np.int64); hi = np.full(N, -1, np.int64)
    seg = np.repeat(np.arange(len(c["snp_pos"])), np.diff(c["col_off"])) // 64
    np.minimum.at(lo, c["col_idx"], seg); np.maximum.at(hi, c["col_idx"], seg)
    return lo, hi


def start_order(c):
    """reads by start position, ties by index: row k of the contig's matrices is the read start_order(c)[k]"""
    return np.lexsort((np.arange(len(c["read_start"])), c["read_start"])).astype(np.int32)


def block_word_ranges(c):
    """per 64-row block of the matrices (rows in start order): first and last word any of its reads is present in"""
    lo, hi = presence_words(c)
    o = start_order(c)
    nb = (len(o) + 63) // 64
    return (np.array([lo[o[64 * b:64 * b + 64]].min() for b in range(nb)]), np.array([hi[o[64 * b:64 * b + 64]].max() for b in range(nb)]))


def tile_words(c, bi, bj):
    """the words K5 walks for the tile of blocks (bi, bj): None if the blocks share none, else (w_begin rounded down to 16, w_end)"""
    lo, hi = block_word_ranges(c)
    b, e = max(lo[bi], lo[bj]), min(hi[bi], hi[bj]) + 1
    if b >= e:
        return None
    return int(b) & ~15, int(min(e, (len(c["snp_pos"]) + 63) // 64))


def presence_is_one_run(c):
    """every read is present at every SNP between its first and its last one (what lets the device build a low-memory contig's graphs)"""
    N = len(c["read_start"])
    seg = np.repeat(np.arange(len(c["snp_pos"])), np.diff(c["col_off"]))
    first = np.full(N, 2 ** 31 - 1, np.int64); last = np.full(N, -1, np.int64); cnt = np.zeros(N, np.int64)
    np.minimum.at(first, c["col_idx"], seg); np.maximum.at(last, c["col_idx"], seg); np.add.at(cnt, c["col_idx"], 1)
    return bool(np.all((cnt == 0) | (cnt == last - first + 1)))


def ambiguous_rows(sim, diff, mask_ids, error_rate):
    """rows of create_read_graph_matrix (separate_reads.cpp:737-815) whose five-neighbour cut-off falls inside a run of equal distances"""
    N = sim.shape[0]
    mask = np.zeros(N, bool); mask[mask_ids] = True
    below = np.float32(1) - np.float32(error_rate) * np.float32(2)
    n_amb = 0
    for r1 in mask_ids:
        s = np.where(mask, sim[:, r1], 0); d = np.where(mask, diff[:, r1], 0)
        s[r1] = 0; d[r1] = 0
        dist = np.zeros(N, np.float32)
        ok = s > 0
        dist[ok] = np.float32(1) - np.maximum(0, d[ok] - 1).astype(np.float32) / (s[ok] + d[ok]).astype(np.float32)
        far = mask & (s + d < 0.7 * (s[ok].max() if ok.any() else 0)); far[r1] = False
        dist[far] = 0
        top = np.sort(dist)[::-1]
        above = np.float32(1)
        if N > 1:
            above = np.float32(top[0] - np.float32(np.float32(top[0] - top[1]) * np.float32(3)))
        if above == 1:
            k = int(np.sum(top == 1))
            if k < N:
                above = top[min(k + 4, N - 1)]
        cand = mask & (dist > below)
        always = cand & ((dist == 1) | (dist >= above))
        rest = np.sort(dist[cand & ~always])[::-1]
        need = 5 - int(always.sum())
        if need > 0 and len(rest) > need and rest[need - 1] == rest[need]:
            n_amb += 1
    return n_amb


def to_i64(case, seed=12345):
    """the case as tests/harness/host_harness graph_taps reads it"""
    parts = [np.array([len(case["contigs"]), case["window"], 1 if case["low_memory"] else 0, seed, int(np.float32(case["error_rate"]).view(np.uint32))], np.int64)]
    for c in case["contigs"]:
        parts.append(np.array([c["length"], len(c["read_start"]), len(c["snp_pos"]), len(c["col_idx"])], np.int64))
        parts += [np.asarray(c[k]).astype(np.int64) for k in ("read_start", "read_end", "snp_pos", "snp_ref", "snp_alt", "col_off", "col_idx", "col_code")]
    return np.concatenate(parts)


def from_i64(out):
    """host_harness graph_taps' answer -> (rows on host, [window dicts: contig, kind, ids, nbr (list of lists of read ids)])"""
    W, on_host = int(out[0]), int(out[1])
    at = 2
    wins = []
    for _ in range(W):
        c, kind, m = (int(x) for x in out[at:at + 3]); at += 3
        ids = out[at:at + m].astype(np.int32); at += m
        nbr = []
        for _ in range(m):
            d = int(out[at]); nbr.append(out[at + 1:at + 1 + d].tolist()); at += 1 + d
        wins.append({"contig": c, "kind": kind, "ids": ids, "nbr": nbr})
    assert at == len(out)
    return on_host, wins


# ---- what the oracle says (oracle_lib is passed in: this module itself needs numpy only) ----
_oracle = {}


def oracle_masks(ol, name):
    """per contig of the case: the read lists of its graph windows, from the oracle's separate_reads_on_contig (contig by contig, as the reference goes)"""
    key = ("masks", name)
    if key not in _oracle:
        case = get(name)
        out = []
        for c in case["contigs"]:
            if len(c["snp_pos"]) == 0:
                out.append([]); continue
            t = ol.sr_contig_taps(c, case["window"], case["error_rate"], low_memory=case["low_memory"] or coverage_above_1000(c))
            out.append([t["mask_ids"][t["tap_row0"][k]:t["tap_row0"][k + 1]] for k in range(len(t["tap_start"]))])
        _oracle[key] = out
    return _oracle[key]


def oracle_simdiff(ol, name, ci):
    """(sim, diff) [N, N] of contig ci in read order, from the oracle's list_similarities_and_differences; computed once, never changed"""
    key = ("simdiff", name, ci)
    if key not in _oracle:
        c = get(name)["contigs"][ci]
        sim, diff = ol.simdiff(len(c["read_start"]), c["snp_ref"], c["snp_alt"], c["col_off"], c["col_idx"], c["col_code"])
        sim.setflags(write=False); diff.setflags(write=False)
        _oracle[key] = (sim, diff)
    return _oracle[key]


def oracle_graph(ol, name, ci, ids, kind):
    """neighbour lists (read ids) of the window of contig ci whose mask is `ids`, one list per read of `ids`: create_read_graph_matrix for kind 0,
    create_read_graph_low_memory for the two low-memory kinds"""
    case = get(name)
    c = case["contigs"][ci]
    N = len(c["read_start"])
    mask = np.zeros(N, np.uint8); mask[ids] = 1
    if kind == 0:
        sim, diff = oracle_simdiff(ol, name, ci)
        adj = ol.read_graph(sim, diff, mask, case["error_rate"])
    else:
        adj = ol.read_graph_low_memory(N, c["snp_ref"], c["snp_alt"], c["col_off"], c["col_idx"], c["col_code"], mask, case["error_rate"])
    assert all(len(adj[r]) == 0 for r in np.nonzero(mask == 0)[0])
    return [adj[int(r)] for r in ids]
