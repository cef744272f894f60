"""Stage-4 inputs for the clustering chain -- k_cw_seed_sets, k_cw_seeded_lanes / _rows / _wave and k_window_tail (hs_kernels_cw.hip), routed by cw_chain
(hs_sr_backend.inc) -- built directly, at the read counts and table sizes where the chain takes another kernel, another path inside a kernel, or hands a
window back to the host. Used by tests/test_cpu_chain_cases.py (which proves with the oracle alone that every case is what it claims, and derives the route
counters the device must report) and tests/test_gpu_chain_routes.py.

A case is {"contigs": [contig dict ...], "window": w, "error_rate": e}; a contig dict is what graph_cases builds, plus "claims": what the window with SNPs of
that contig was designed to be (see CLAIM_KEYS). Every contig is graph_cases.one_window_contig's: 2150 positions, one window [0, 2000) with SNPs whose mask
is exactly the m reads that span the contig (the others end at 1200 or start at 1201), the m reads dealt to h haplotypes of equal size."""
import numpy as np

import graph_cases as gc

# ---- the constants the routes hang on, each with the line it comes from ----
LANES_CAP = 64            # hs_sr_backend.inc:596 `const int lanes_cap = 64` -- one run per lane up to here; k_window_tail keeps the labels in registers up to the same count
CWL_SLOTS = 16            # hs_kernels_cw.hip:495 `#define HS_CWL_SLOTS 16` -- labels alive after seeding a lane run may have; more: the overflow list (:537)
CWR_CAP = 255             # hs_kernels_cw.hip:31 `#define HS_CWR_CAP 255` -- row-packed units up to here, one wavefront per run above (hs_sr_backend.inc:625-628)
ROW_UNIT = 8              # hs_sr_backend.inc:630 `i += 8` -- runs per row-packed unit
WAVE_LDS_NODES = 96 * 1024 // 8 // 64 * 64      # hs_sr_backend.inc:636 `lds_nodes(max_m_big, 2, 96 * 1024)` = 12288 -- above: k_cw_seeded_wave in global scratch
TAIL_LDS_NODES = 56 * 1024 // 28 // 64 * 64     # hs_sr_backend.inc:642 `lds_nodes(max_m_chain, 7, 56 * 1024)` = 2048 -- above: the tail in global scratch
SPEC_LABELS = 8           # hs_kernels_cw.hip:725 `#define HS_CW_SPEC_LABELS 8` -- cw_run_sets: speculative sweep up to here, walked sweep above
FIN_KCAP = 16             # hs_kernels_cw.hip:25 `#define HS_FIN_KCAP 16` -- labels behind the third run's renumbering; more: host (:950, :1052)
FIN_GCAP = 8              # hs_kernels_cw.hip:26 `#define HS_FIN_GCAP 8` -- clusters entering merge_wrongly_split_haplotypes; more: host (:1166)
FIN_LCAP = 16             # hs_kernels_cw.hip:27 `#define HS_FIN_LCAP 16` -- entries of its links map; more: host (:1381)
TAIL_BATCH = 8            # hs_kernels_cw.hip:30 `#define HS_TAIL_BATCH 8` -- SNP columns in flight in merge_wrongly_split_haplotypes
FAST_COLUMN = 64          # hs_kernels_cw.hip:1303 `n > 64` -- a SNP column of at most 64 entries takes the per-column fast path (snp_fast), a deeper one snp_deep
TAIL_MAP_EXTRA = 1024     # hs_kernels_cw.hip:29 `#define HS_TAIL_MAP_EXTRA 1024` -- bytes of the read id -> cluster map of a narrow window (:1178-1179): id range up to here
PAIR_GAP = 10             # separate_reads.cpp:1126 `snp.pos - pos_of_last_incompatibilities[..][..] > 10`; the same gap decides which SNPs seed a run (:1675)
MIN_CLUSTER = 5           # separate_reads.cpp:936-938 clusters under 5 reads become -1

ROUTE_KEYS = ("all_lanes", "runs_lanes", "runs_overflow", "runs_rows", "units_rows", "runs_wave", "runs_wave_scratch", "tail_narrow", "tail_lds", "tail_scratch",
              "cap_tail")
# what a contig may claim about its window (None / absent: not claimed): the test compares each with what the oracle says
CLAIM_KEYS = ("m", "runs", "kc", "g", "n_links", "merged", "vetoed", "labels", "all_unclustered", "n_visit0", "overflow_runs", "codes", "depths",
              "snps_inside", "id_range", "gap_pairs", "tie_break", "key_variants", "split_variants")


def spread(S, step=30, first=500):
    """S positions `step` apart from `first`: each seeds a run (step > PAIR_GAP)"""
    return (first + step * np.arange(S)).astype(np.int32)


def grouped(R, per=4, first=500, step=40):
    """R groups of `per` SNPs at consecutive positions, `step` apart: the first of every group seeds a run, the others lie within PAIR_GAP of it"""
    return np.concatenate([first + step * g + np.arange(per) for g in range(R)]).astype(np.int32)


def twins(d):
    """allele patterns in which haplotype 2 k + 1 differs from haplotype 2 k at d SNPs only: clusters the per-SNP runs split and the graph links"""
    def make(rng, S, n_hap):
        p = rng.integers(0, 2, (S, n_hap))
        for k in range(1, n_hap, 2):
            p[:, k] = p[:, k - 1]
            flip = rng.permutation(S)[:d]
            p[flip, k] ^= 1
        return p
    return make


def paired(diff_at):
    """independent draws, but haplotype 1 is haplotype 0 except at the SNPs diff_at: two clusters whose majority bases differ exactly there"""
    def make(rng, S, n_hap):
        p = rng.integers(0, 2, (S, n_hap))
        p[:, 1] = p[:, 0]
        p[list(diff_at), 1] ^= 1
        return p
    return make


def sole_run(R, k, per=4):
    """for grouped(R, per): two haplotypes that agree at every SNP that seeds a run except the one of run k, and differ at every other SNP: the graph
    keeps them apart, and run k alone tells them apart in the merged-ids key"""
    def make(rng, S, n_hap):
        assert S == R * per and n_hap == 2
        p = np.zeros((S, 2), np.int64)
        p[:, 0] = rng.integers(0, 2, S)
        p[:, 1] = p[:, 0] ^ 1
        seeds = per * np.arange(R)
        p[seeds, 1] = p[seeds, 0]
        p[per * k, 1] ^= 1
        return p
    return make


def forced(rows):
    """independent draws, but at SNP s the haplotypes carry rows[s]: clusters known to differ there"""
    def make(rng, S, n_hap):
        p = rng.integers(0, 2, (S, n_hap))
        for k, row in rows.items():
            p[k] = row
        return p
    return make


def window(seed, m, h, snp_pos, extra=0, noise=0.02, third=0.0, pattern=None, full_ids=None, length=None, **claims):
    """one contig whose window holds exactly m reads of h haplotypes (and `extra` reads outside the mask)"""
    rng = np.random.default_rng(seed)
    snp_pos = np.asarray(snp_pos, np.int32)
    assert 400 <= snp_pos[0] and snp_pos[-1] < 1990 and np.all(np.diff(snp_pos) > 0)      # (separate_reads.cpp:1593-1607: no SNP the mask's ends are moved past)
    assert extra == 0 or (snp_pos[0] <= 1200 < snp_pos[-1])
    c = gc.one_window_contig(rng, m + extra, m, len(snp_pos), snp_pos=snp_pos, balanced=True, n_hap=h, noise=noise, third=third, pattern=pattern,
                             full_ids=full_ids, length=length)
    c["claims"] = dict({"m": m}, **claims)
    return c


def _case(contigs):
    return {"contigs": contigs, "window": gc.WINDOW, "error_rate": 0.05}


def set_column_codes(c, s, n_codes, rng):
    """SNP column s: its entries of reads that span the contig get exactly n_codes distinct codes (bytes from 'a' on, every one used)"""
    a, b = int(c["col_off"][s]), int(c["col_off"][s + 1])
    full = (c["read_start"][c["col_idx"][a:b]] <= c["snp_pos"][0]) & (c["read_end"][c["col_idx"][a:b]] >= c["snp_pos"][-1])
    n = int(full.sum())
    assert n >= n_codes
    codes = np.concatenate((np.arange(n_codes), rng.integers(0, n_codes, n - n_codes)))
    c["col_code"][a:b][full] = (97 + codes[rng.permutation(n)]).astype(np.uint8)


def retire_reads(c, n_keep):
    """all but n_keep of the reads outside the mask are moved behind the last SNP and taken out of every column: read ids that lie in no column"""
    full = (c["read_start"] <= c["snp_pos"][0]) & (c["read_end"] >= c["snp_pos"][-1])
    dead = np.flatnonzero(~full)[n_keep:]
    c["read_start"][dead] = c["snp_pos"][-1] + 100; c["read_end"][dead] = c["length"] - 100
    keep = ~np.isin(c["col_idx"], dead)
    seg = np.repeat(np.arange(len(c["snp_pos"])), np.diff(c["col_off"]))
    c["col_idx"] = c["col_idx"][keep]; c["col_code"] = c["col_code"][keep]
    c["col_off"] = np.concatenate(([0], np.cumsum(np.bincount(seg[keep], minlength=len(c["snp_pos"]))))).astype(np.int64)


def pad_column(c, s, depth):
    """SNP column s is cut down to `depth` entries: entries of reads outside the mask are dropped from its end (those reads skip the position)"""
    a, b = int(c["col_off"][s]), int(c["col_off"][s + 1])
    idx = c["col_idx"][a:b]
    full = (c["read_start"][idx] <= c["snp_pos"][0]) & (c["read_end"][idx] >= c["snp_pos"][-1])
    drop = np.flatnonzero(~full)[::-1][:(b - a) - depth]
    assert (b - a) - len(drop) == depth
    keep = np.ones(len(c["col_idx"]), bool); keep[a + drop] = False
    c["col_idx"] = c["col_idx"][keep]; c["col_code"] = c["col_code"][keep]
    c["col_off"] = c["col_off"].copy(); c["col_off"][s + 1:] -= len(drop)


def border_column(c, s):
    """SNP column s: the haplotype of the column's last entry (the read with the highest index, which spans the contig) gets its majority base at twice
    the count of its runner-up, the SNP's third allele, the last entry among the majority: a cluster whose majority base stands with that entry and falls
    without it (separate_reads.cpp:1093 `secondMax * 2 > max`)"""
    a, b = int(c["col_off"][s]), int(c["col_off"][s + 1])
    idx = c["col_idx"][a:b]
    full = (c["read_start"][idx] <= c["snp_pos"][0]) & (c["read_end"][idx] >= c["snp_pos"][-1])
    assert full[-1]
    own = np.flatnonzero(full & (c["hap"][idx] == c["hap"][idx[-1]]))
    code = c["col_code"][a:b]
    major = np.uint8(np.argmax(np.bincount(code[own], minlength=256)))
    other = c["snp_alt"][s] if major == c["snp_ref"][s] else c["snp_ref"][s]
    assert major in (c["snp_ref"][s], c["snp_alt"][s])
    k = len(own) // 3
    code[own] = major
    code[own[:k]] = c["snp_third"][s]
    code[own[k:len(own) - 2 * k]] = other
    assert np.sum(code[own] == major) == 2 * k and np.sum(code[own] == c["snp_third"][s]) == k and code[-1] == major


# ---- the cases ----
def case_narrow():
    """every window at most 64 reads: cw_chain's all_lanes branch, k_cw_seeded_lanes, the register tail"""
    return _case([
        window(201, 1, 1, spread(5, 200), extra=6, runs=5, kc=0, g=0, all_unclustered=True),
        window(202, 4, 1, spread(5, 200), extra=6, runs=5, kc=0, g=0, all_unclustered=True),      # every cluster under MIN_CLUSTER reads
        window(203, 5, 1, spread(5, 200), extra=6, runs=5, kc=1, g=1, labels=1),
        window(204, 64, 8, spread(40), extra=9, runs=40, kc=8, g=8, n_links=0, labels=8),      # SPEC_LABELS alive: the speculative sweep; FIN_GCAP clusters: device
        window(205, 56, 8, spread(40), extra=9, runs=40, kc=8, g=8, labels=8),
        window(206, 63, 9, spread(40), extra=9, runs=40, kc=9, g=9, labels=9),                 # the walked sweep; host
        window(207, 60, 12, spread(40), extra=9, runs=40, kc=12, g=12, labels=12),             # host
        window(208, 12, 2, spread(6, 200), extra=6, third=1.0, runs=6, n_visit0=True),           # third alleles only: no read has a neighbour
        # noisy windows in which a visit of the tail's runs meets equal counts: the lowest of the equal labels wins (cluster_graph.cpp:272-279); few
        # labels alive (speculative sweep) and more than SPEC_LABELS (walked sweep, FIN_LCAP links with g <= FIN_GCAP: device)
        window(0, 40, 2, spread(8, 150), extra=6, noise=0.1, runs=8, tie_break=True),
        window(3, 56, 2, spread(8, 150), extra=6, noise=0.15, runs=8, tie_break=True),
        window(0, 60, 9, spread(12, 100), extra=6, noise=0.05, runs=12, kc=9, g=7, n_links=16, tie_break=True),
    ])


def case_mixed():
    """m = 64, 65, 255, 256, 300 in one call: the mixed host branch, all three run kernels at both edges; run counts 1 .. 21 and windows past 53 runs.
    The windows behind the first ten hold two haplotypes that one run alone tells apart in the merged-ids key (sole_run): the 17th (the key's 16 + 1
    tail), the 21st (16 + 4 + 1), and, among 60 and 62 runs, the 56th / 58th -- a key without that run gives another third run -- and the first: there the
    reference's double key has rounded the run away by the time the last is added, so the two haplotypes share a key, and a key summed exactly gives
    another third run (key_variants, asserted in tests/test_cpu_chain_cases.py)"""
    shapes = [(64, 1), (64, 17), (65, 9), (65, 8), (255, 3), (255, 16), (256, 4), (256, 15), (300, 5), (300, 21)]
    cs = [window(220 + k, m, 3, grouped(R), runs=R) for k, (m, R) in enumerate(shapes)]
    sole = lambda seed, m, R, k, v: window(seed, m, 2, grouped(R, first=420, step=1400 // R), extra=5, pattern=sole_run(R, k), runs=R, key_variants=[v])
    cs += [sole(400, 64, 17, 16, {"omit": 16}), sole(400, 65, 21, 20, {"omit": 20}), sole(400, 255, 21, 16, {"omit": 16}),
           sole(400, 64, 60, 55, {"omit": 55}), sole(400, 256, 62, 57, {"omit": 57}),
           sole(401, 64, 60, 0, {"exact": True}), sole(401, 256, 62, 0, {"exact": True})]
    return _case(cs)


def case_tables():
    """wide windows either side of FIN_KCAP, FIN_GCAP and FIN_LCAP; the seeds come from a search with the oracle"""
    return _case([
        window(2, 128, 16, spread(40), noise=0.08, pattern=twins(4), runs=40, kc=16, g=8, n_links=0),      # kc == FIN_KCAP: device
        window(240, 102, 17, spread(40), runs=40, kc=17, g=17),                                             # kc == FIN_KCAP + 1: host
        window(241, 72, 8, spread(40), runs=40, kc=8, g=8),                                                 # g == FIN_GCAP: device
        window(242, 81, 9, spread(40), runs=40, kc=9, g=9),                                                 # g == FIN_GCAP + 1: host
        window(5, 105, 5, spread(12, 1400 // 12), noise=0.1, runs=12, g=5, n_links=16, vetoed=13),          # n_links == FIN_LCAP: device
        window(4, 125, 6, spread(6, 1400 // 6), noise=0.1, runs=6, g=5, n_links=18),                        # the least above FIN_LCAP a symmetric graph gives: host
        window(3, 128, 16, spread(40), noise=0.12, pattern=twins(2), runs=40, kc=11, g=8, n_links=2, merged=1, vetoed=0),      # a link applied: device
        window(2, 160, 16, spread(40), noise=0.12, pattern=twins(4), runs=40, kc=12, g=8, n_links=2, merged=0, vetoed=2),      # links refused: device
    ])


def case_alleles():
    """seeding columns with exactly CWL_SLOTS and CWL_SLOTS + 1 distinct codes among the masked reads, at m <= 64 (overflow list) and at m = 130 and 256
    (k_cw_seeded_rows / _wave seed from the columns themselves)"""
    cs = []
    for k, m in enumerate((40, 64, 130, 256)):
        c = window(250 + k, m, 3, spread(6, 200), extra=7, runs=6, codes={1: CWL_SLOTS, 3: CWL_SLOTS + 1, 4: CWL_SLOTS + 1}, overflow_runs=2 if m <= LANES_CAP else 0)
        rng = np.random.default_rng(260 + k)
        for s, n in c["claims"]["codes"].items():
            set_column_codes(c, s, n, rng)
        cs.append(c)
    return _case(cs)


def case_columns():
    """narrow windows at the column forks of merge_wrongly_split_haplotypes: depths FAST_COLUMN and FAST_COLUMN + 1, TAIL_BATCH - 1 .. 2 TAIL_BATCH + 1 columns
    inside the window, read id ranges TAIL_MAP_EXTRA and TAIL_MAP_EXTRA + 1, SNP pairs PAIR_GAP and PAIR_GAP + 1 apart"""
    cs = []
    c = window(270, 50, 3, spread(8, 150), extra=40, runs=8, depths={1: FAST_COLUMN, 2: FAST_COLUMN + 1, 5: FAST_COLUMN, 6: FAST_COLUMN + 1}, snps_inside=8)
    for s, d in c["claims"]["depths"].items():
        pad_column(c, s, d)
    cs.append(c)
    # two clusters whose majority bases differ at two SNPs only, and a link between them: refused for the two (an incompatibility count of 2), applied if
    # the walk loses one of the two columns (split_variants: forms of the merge step that must give other finished labels; the seeds come from a search)
    for seed, noise, S, other, k in ((604, 0.05, TAIL_BATCH - 1, 1, 6), (603, 0.02, TAIL_BATCH, 2, 7), (620, 0.08, TAIL_BATCH + 1, 3, 8),
                                     (604, 0.05, 2 * TAIL_BATCH + 1, 2, 16), (604, 0.05, 2 * TAIL_BATCH + 1, 2, 8), (604, 0.05, 2 * TAIL_BATCH + 1, 2, 7)):
        cs.append(window(seed, 48, 2, spread(S, 720 // (S - 1) + 1), extra=8, noise=noise, pattern=paired((other, k)), runs=S, snps_inside=S, g=2, n_links=2,
                         merged=0, vetoed=2, split_variants=[{"skip_col": k}]))
    # the same, the second of the two SNPs behind a clump of four that counts once (PAIR_GAP): a column of FAST_COLUMN / FAST_COLUMN + 1 entries in which
    # the majority base of the cluster of the last entry stands with that entry only (border_column)
    base = spread(24, 50, 450)
    pos = np.sort(np.concatenate((base, base[3] + 1 + np.arange(3))))
    for d in (FAST_COLUMN, FAST_COLUMN + 1):
        c = window(701, 48, 2, pos, extra=60, pattern=paired((3, 4, 5, 6, 17)), runs=24, depths={17: d}, g=2, n_links=2, merged=0, vetoed=2,
                   split_variants=[{"cut_depth": d}])
        pad_column(c, 17, d); border_column(c, 17)
        if d == FAST_COLUMN:      # every column at FAST_COLUMN entries: no batch of TAIL_BATCH columns holds a deep one, so none is walked one by one (:1307)
            for s in range(len(pos)):
                pad_column(c, s, d)
            c["claims"]["depths"] = {s: d for s in range(len(pos))}
        cs.append(c)
    for k, lo in enumerate((6, 5)):      # reads lo .. 1029 span the contig: an id range of 1024 (the byte map) and of 1025 (bisection)
        rng = np.random.default_rng(280 + k)
        ids = np.concatenate(([lo], lo + 1 + rng.permutation(1029 - lo - 1)[:38], [1029]))
        c = window(282 + k, 40, 3, spread(8, 150), extra=990, full_ids=np.sort(ids), length=3000, runs=8, id_range=1029 - lo + 1)
        retire_reads(c, 12)      # (columns of at most FAST_COLUMN entries: the fast path is the one that reads the map)
        cs.append(c)
    pos = np.array([500, 700, 710, 900, 911, 1300, 1500], np.int32)      # 700 / 710: PAIR_GAP apart; 900 / 911: PAIR_GAP + 1
    cs.append(window(290, 48, 4, pos, extra=8, pattern=forced({1: [0, 1, 0, 1], 2: [0, 1, 0, 1], 3: [0, 0, 1, 1], 4: [0, 0, 1, 1]}), runs=6, gap_pairs=[(1, 2, False), (3, 4, True)], snps_inside=7))
    # two clusters that differ at SNPs 2 and 3 only, PAIR_GAP apart: counted once, the link is applied (with `> 9` twice: refused); PAIR_GAP + 1 apart:
    # counted twice, refused (with `> 11` once: applied)
    for d, v, merged in ((PAIR_GAP, 9, 1), (PAIR_GAP + 1, 11, 0)):
        pos = np.array([500, 650, 800, 800 + d, 1000, 1250, 1400, 1550], np.int32)
        cs.append(window(514, 48, 2, pos, extra=8, pattern=paired((2, 3)), runs=7 + (d > PAIR_GAP), gap_pairs=[(2, 3, d > PAIR_GAP)], g=2, n_links=2, merged=merged,
                         vetoed=2 - 2 * merged, split_variants=[{"gap": v}]))
    return _case(cs)


def case_scratch():
    """m = TAIL_LDS_NODES and TAIL_LDS_NODES + 1 in one call: cap_tail = 2048, one tail in LDS and one in global scratch (contigs long enough for a coverage
    under 1000: the matrix path)"""
    return _case([window(300 + k, m, 3, spread(5, 200), extra=7, length=4500, runs=5) for k, m in enumerate((TAIL_LDS_NODES, TAIL_LDS_NODES + 1))])


def case_scratch_alone():
    """m = TAIL_LDS_NODES alone: the widest window whose tail stays in LDS, with nothing wider in the call"""
    return _case([window(300, TAIL_LDS_NODES, 3, spread(5, 200), extra=7, length=4500, runs=5)])


CASES = {"narrow": case_narrow, "mixed": case_mixed, "tables": case_tables, "alleles": case_alleles, "columns": case_columns, "scratch": case_scratch,
         "scratch_alone": case_scratch_alone}
_made = {}
_oracle = {}


def get(name):
    """the case, built once per process (read-only)"""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def oracle_taps(ol, name):
    """per contig of the case: oracle_lib.sr_contig_taps (the oracle's separate_reads_on_contig with its taps on), computed once, never changed"""
    if name not in _oracle:
        case = get(name)
        _oracle[name] = [ol.sr_contig_taps(c, case["window"], case["error_rate"]) for c in case["contigs"]]
    return _oracle[name]


def window_facts(t):
    """what the oracle says about the one window with SNPs of a contig: m, runs, kc, g, n_links, n_merged, n_vetoed, and whether the device hands it back"""
    assert len(t["tap_start"]) == 1
    f = {"m": int(t["tap_row0"][1]), "runs": int(t["run_begin"][1])}
    for k in ("kc", "g", "n_links", "n_merged", "n_vetoed"):
        f[k] = int(t[k][0])
    f["on_host"] = f["runs"] > 0 and (f["kc"] > FIN_KCAP or f["g"] > FIN_GCAP or f["n_links"] > FIN_LCAP)
    return f


def seeded_labels_alive(c, t):
    """per run of the window: labels alive after seeding (separate_reads.cpp:1678-1691) = distinct codes of the masked reads in the seeding column + masked
    reads that are not in it"""
    ids = t["mask_ids"]
    out = []
    for s in t["run_snp"]:
        a, b = int(c["col_off"][s]), int(c["col_off"][s + 1])
        inm = np.isin(c["col_idx"][a:b], ids)
        out.append(len(set(c["col_code"][a:b][inm].tolist())) + len(ids) - int(inm.sum()))
    return out


def expected_routes(facts, alive):
    """the route counters of a call from (m, runs) of its chain windows and the labels alive per run: cw_chain's list building, restated"""
    ws = [f for f in facts if f["runs"] > 0]
    ms = [f["m"] for f in ws]
    r = dict.fromkeys(ROUTE_KEYS, 0)
    r["all_lanes"] = int(all(m <= LANES_CAP for m in ms))
    for f, al in zip(facts, alive):
        if f["runs"] == 0:
            continue
        if f["m"] <= LANES_CAP:
            r["runs_lanes"] += f["runs"]; r["runs_overflow"] += sum(1 for a in al if a > CWL_SLOTS)
        elif f["m"] <= CWR_CAP:
            r["runs_rows"] += f["runs"]; r["units_rows"] += -(-f["runs"] // ROW_UNIT)
        else:
            r["runs_wave"] += f["runs"]
    big = [m for m in ms if m > CWR_CAP]
    cap_big = min((max(big + [1]) + 63) // 64 * 64, WAVE_LDS_NODES)
    r["runs_wave_scratch"] = sum(f["runs"] for f in ws if f["m"] > CWR_CAP and f["m"] > cap_big)
    r["cap_tail"] = min((max(ms + [1]) + 63) // 64 * 64, TAIL_LDS_NODES)
    for m in ms:
        r["tail_narrow" if m <= LANES_CAP else ("tail_scratch" if m > r["cap_tail"] else "tail_lds")] += 1
    return r
