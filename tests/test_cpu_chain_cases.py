"""The cases of tests/chain_cases.py are what they claim to be, shown with the oracle and numpy alone (no GPU): every window's read count, run count, the
table sizes of its finalize_clustering (kc, g, n_links, n_merged, n_vetoed from the oracle's taps), column depths, codes per seeding column, read id ranges --
and, from those numbers and the constants restated in chain_cases.py, the route counters and the number of windows handed back to the host that
tests/test_gpu_chain_routes.py expects of the device."""
import numpy as np
import pytest

import chain_cases as cc
import graph_cases as gc
import oracle_lib as ol


@pytest.fixture(scope="module", autouse=True)
def _artefacts(built):
    return built


def _spanning(c):
    return np.flatnonzero((c["read_start"] <= c["snp_pos"][0]) & (c["read_end"] >= c["snp_pos"][-1]))


def _majorities(c, s, ids, labels):
    """cluster -> majority code at SNP s (separate_reads.cpp:1085-1099: none when the runner-up has more than half of it or it has less than half the reads)"""
    a, b = int(c["col_off"][s]), int(c["col_off"][s + 1])
    lab = dict(zip(ids.tolist(), labels.tolist()))
    out = {}
    for cl in set(labels[labels >= 0].tolist()):
        codes = [int(x) for r, x in zip(c["col_idx"][a:b].tolist(), c["col_code"][a:b].tolist()) if lab.get(r, -2) == cl]
        cnt = sorted(np.bincount(codes, minlength=256).tolist(), reverse=True)
        if codes and not (cnt[1] * 2 > cnt[0] or len(codes) * 0.5 > cnt[0]):
            out[cl] = int(np.argmax(np.bincount(codes, minlength=256)))
    return out


def _cw(adj, init, order, high):
    """chinese_whispers (cluster_graph.cpp:240-310) restated: a node takes the most frequent label among its neighbours, the lowest of equals -- or,
    with `high`, the highest: the rule a case must be able to tell from the right one"""
    lab = list(init)
    changes, iters = 3, 0
    while changes > 2 and iters < 15:
        changes = 0
        for i in order:
            if lab[i] == -2:
                continue
            cnt = {}
            for nb in adj[i]:
                if lab[nb] >= 0:
                    cnt[lab[nb]] = cnt.get(lab[nb], 0) + 1
            if cnt:
                top = max(cnt.values())
                ties = [l for l, v in cnt.items() if v == top]
                best = max(ties) if high else min(ties)
                changes += lab[i] != best
                lab[i] = best
        iters += 1
    return lab


def _graph(c, ids, error_rate):
    """the window's read graph: neighbour lists per read of the contig"""
    N = len(c["read_start"])
    sim, diff = ol.simdiff(N, c["snp_ref"], c["snp_alt"], c["col_off"], c["col_idx"], c["col_code"])
    mask = np.zeros(N, np.uint8); mask[ids] = 1
    return ol.read_graph(sim, diff, mask, error_rate)


def _third_run(c, t, error_rate, high, seed=12345, omit=None, exact=False):
    """the labels of the third run from the per-SNP runs' labels (merge_clusterings + finalize_clustering up to :970), restated.
    omit: a run left out of the merged-ids key; exact: the key summed in integers instead of doubles -- keys a case must be able to tell from the right one"""
    N = len(c["read_start"])
    ids = t["mask_ids"]
    m, runs = len(ids), int(t["run_begin"][1])
    mask = np.zeros(N, np.uint8); mask[ids] = 1
    adj = _graph(c, ids, error_rate)
    order = ol.shuffled_order(N, seed).tolist()
    run = np.full((runs, N), -2, np.int64); run[:, ids] = t["run_labels"].reshape(runs, m)
    seen, ints = {}, []
    for r in range(N):
        agg = 0 if exact else 0.0
        for i in range(runs):
            if i != omit:
                agg += int(run[i, r]) * 2 ** i if exact else float(run[i, r]) * 2.0 ** i
        ints.append(seen.setdefault(agg, len(seen)) if mask[r] else -2)
    lab = _cw(adj, ints, order, high)
    size = {}
    for l in lab:
        size[l] = size.get(l, 0) + 1
    lab = [-1 if l != -2 and size[l] < cc.MIN_CLUSTER else l for l in lab]
    to_hap = {}
    lab = [to_hap.setdefault(l, len(to_hap)) if l > -1 else l for l in lab]
    return np.array(_cw(adj, lab, order, high))[ids]


def _merge_split(c, t, error_rate, window, gap=cc.PAIR_GAP, skip_col=None, cut_depth=None):
    """merge_wrongly_split_haplotypes (separate_reads.cpp:1007-1327) restated, from the labels it is given to the window's finished labels.
    gap: the distance a SNP must exceed from the pair's last counted one; skip_col: an in-window column (counted from 0) left out of the walk;
    cut_depth: columns of exactly this many entries lose their last one -- the off-by-one forms a case must be able to tell from the right one"""
    N = len(c["read_start"])
    ids = t["mask_ids"]
    lab = np.full(N, -2, np.int64); lab[ids] = t["split"]
    groups = sorted(set(lab[lab >= 0].tolist()))
    if len(groups) <= 1:
        return np.zeros(len(ids), np.int64)
    index = {}
    for l in lab.tolist():
        if l >= 0:
            index.setdefault(l, len(index))
    G = len(groups)
    incompat = np.zeros((G, G), np.int64); pos_last = np.full((G, G), -10, np.int64)
    k_in = 0
    for s, pos in enumerate(c["snp_pos"].tolist()):
        if not 0 <= pos < window:
            continue
        k_in += 1
        if k_in - 1 == skip_col:
            continue
        a, b = int(c["col_off"][s]), int(c["col_off"][s + 1])
        if b - a == cut_depth:
            b -= 1
        counts = {}
        for r, x in zip(c["col_idx"][a:b].tolist(), c["col_code"][a:b].tolist()):
            if lab[r] >= 0:
                counts.setdefault(int(lab[r]), {}).setdefault(x, 0)
                counts[int(lab[r])][x] += 1
        maj = {}
        for cl, cnt in counts.items():
            v = sorted(cnt.values(), reverse=True) + [0]
            tied_or_weak = v[1] * 2 > v[0] or sum(cnt.values()) * 0.5 > v[0]
            maj[cl] = 32 if tied_or_weak else max(cnt, key=cnt.get)
        if len(set(x for x in maj.values() if x != 32)) <= 1:
            continue
        for g1 in groups:
            for g2 in groups:
                m1, m2 = maj.setdefault(g1, 0), maj.setdefault(g2, 0)      # (a cluster absent from the column: operator[] leaves 0 there)
                if m1 != 32 and m2 != 32 and g1 > g2 and m1 != m2 and pos - pos_last[index[g1], index[g2]] > gap:
                    incompat[index[g1], index[g2]] += 1; incompat[index[g2], index[g1]] += 1
                    pos_last[index[g1], index[g2]] = pos; pos_last[index[g2], index[g1]] = pos
    adj = _graph(c, ids, error_rate)
    links, links_in = {}, {}
    for k in range(len(adj)):
        for row in adj[k]:
            c1, c2 = int(lab[row]), int(lab[k])
            if c1 != c2:
                links[(c1, c2)] = links.get((c1, c2), 0) + 1
            links_in[c1] = links_in.get(c1, 0) + 1
    ratio = sorted(((n / links_in[p[0]], p) for p, n in sorted(links.items())), key=lambda x: -x[0])
    o2n = {g: g for g in groups}; o2n[-1] = -1; o2n[-2] = -2
    for r, (c1, c2) in ratio:
        if not r > 0.01 or o2n[c1] == o2n[c2]:
            continue
        bad = any(incompat[index[g1], index[g2]] > 1 for g1 in groups if o2n[g1] == o2n[c1] for g2 in groups if o2n[g2] == o2n[c2])
        if not bad:
            for g2 in groups:
                if o2n[g2] == o2n[c2]:
                    o2n[g2] = o2n[c1]
    new = {}
    for g in groups:
        new.setdefault(o2n[g], len(new))
    for g in groups:
        o2n[g] = new[o2n[g]]
    return np.array([o2n[l] for l in lab[ids].tolist()])


def analyse(name):
    """-> (facts per contig, expected route counters, expected n_windows_finished_on_host), with every claim of the case asserted on the way"""
    case = cc.get(name)
    taps = cc.oracle_taps(ol, name)
    facts, alive = [], []
    for ci, (c, t) in enumerate(zip(case["contigs"], taps)):
        where = (name, ci)
        assert not gc.coverage_above_1000(c), where                     # the matrix path: the oracle call above is the reference's
        f = cc.window_facts(t)
        cl = c["claims"]
        assert set(cl) <= set(cc.CLAIM_KEYS), where
        ids = t["mask_ids"]
        third = t["third"]
        final = t["win_labels"][0]
        # m is exact by construction: the mask is the reads that span the contig
        assert f["m"] == cl["m"] and np.array_equal(ids, _spanning(c)), where
        for key, fkey in (("runs", "runs"), ("kc", "kc"), ("g", "g"), ("n_links", "n_links"), ("merged", "n_merged"), ("vetoed", "n_vetoed")):
            if key in cl:
                assert f[fkey] == cl[key], (where, key, f[fkey])
        assert f["n_links"] % 2 == 0, where                              # (the read graph is symmetric: links come in pairs)
        if "labels" in cl:
            assert len(set(final[final >= 0].tolist())) == cl["labels"], where
        if cl.get("all_unclustered"):
            assert np.all(third == -1) and f["kc"] == 0, where
        if cl.get("n_visit0"):
            sim, diff = ol.simdiff(len(c["read_start"]), c["snp_ref"], c["snp_alt"], c["col_off"], c["col_idx"], c["col_code"])
            mask = np.zeros(len(c["read_start"]), np.uint8); mask[ids] = 1
            assert all(len(a) == 0 for a in ol.read_graph(sim, diff, mask, case["error_rate"])), where
        al = cc.seeded_labels_alive(c, t)
        depth = np.diff(c["col_off"])
        for s, n in cl.get("codes", {}).items():
            r = t["run_snp"].tolist().index(s)                           # the column seeds a run
            assert al[r] == n, (where, s, al[r])
            a = int(c["col_off"][s])
            assert np.all(np.isin(ids, c["col_idx"][a:a + depth[s]])), where      # every masked read is in it: the labels alive are its codes
        if "overflow_runs" in cl:
            assert sum(1 for a in al if a > cc.CWL_SLOTS) == cl["overflow_runs"] if f["m"] <= cc.LANES_CAP else cl["overflow_runs"] == 0, where
        for s, d in cl.get("depths", {}).items():
            assert depth[s] == d, (where, s, depth[s])
            a = int(c["col_off"][s])
            assert np.sum(np.isin(c["col_idx"][a:a + d], ids)) == f["m"] < d, where      # the extra entries are reads outside the mask
        if "snps_inside" in cl:
            assert int(np.sum((c["snp_pos"] >= 0) & (c["snp_pos"] < case["window"]))) == cl["snps_inside"] == len(c["snp_pos"]), where
        if "id_range" in cl:
            assert int(ids[-1]) - int(ids[0]) + 1 == cl["id_range"] and f["m"] <= cc.LANES_CAP, where
            assert f["m"] < depth.min() and depth.max() <= cc.FAST_COLUMN and f["g"] >= 2, where      # every column goes through the fast path, which reads the map
        for s1, s2, counted in cl.get("gap_pairs", []):
            assert int(c["snp_pos"][s2]) - int(c["snp_pos"][s1]) == cc.PAIR_GAP + (1 if counted else 0), where
            assert (s2 in t["run_snp"].tolist()) == counted and s1 in t["run_snp"].tolist(), where      # (the same gap rule seeds the runs)
            for s in (s1, s2):
                assert len(set(_majorities(c, s, ids, third).values())) >= 2, (where, s)      # clusters with differing majority bases at both
        if cl.get("tie_break"):
            assert f["m"] <= cc.LANES_CAP and f["runs"] < 53 and not f["on_host"], where      # the register tail's cw_run_sets; the keys are exact
            assert np.array_equal(_third_run(c, t, case["error_rate"], False), third), where   # the restatement is the oracle's ...
            assert not np.array_equal(_third_run(c, t, case["error_rate"], True), third), where      # ... and the other tie-break gives other labels
        for v in cl.get("key_variants", []):
            assert not f["on_host"], where
            assert np.array_equal(_third_run(c, t, case["error_rate"], False), third), where      # the restated key is the oracle's ...
            assert not np.array_equal(_third_run(c, t, case["error_rate"], False, **v), third), (where, v)      # ... and this one gives another third run
        for v in cl.get("split_variants", []):
            assert f["m"] <= cc.LANES_CAP and not f["on_host"], where
            assert np.array_equal(_merge_split(c, t, case["error_rate"], case["window"]), final[ids]), where      # the restated merge step is the oracle's ...
            assert not np.array_equal(_merge_split(c, t, case["error_rate"], case["window"], **v), final[ids]), (where, v)      # ... and this one finishes otherwise
        facts.append(f); alive.append(al)
    return facts, cc.expected_routes(facts, alive), sum(f["on_host"] for f in facts)


def _ms(facts):
    return [f["m"] for f in facts]


def test_narrow_case():
    facts, routes, on_host = analyse("narrow")
    assert _ms(facts) == [1, 4, 5, 64, 56, 63, 60, 12, 40, 56, 60] and max(_ms(facts)) == cc.LANES_CAP
    assert [f["g"] for f in facts[3:7]] == [cc.FIN_GCAP, cc.FIN_GCAP, cc.FIN_GCAP + 1, 12]
    assert [f["kc"] for f in facts[3:7]] == [cc.SPEC_LABELS, cc.SPEC_LABELS, cc.SPEC_LABELS + 1, 12]      # labels alive in the third run, either side of the sweeps' switch
    assert [f["on_host"] for f in facts] == [False] * 5 + [True, True] + [False] * 4
    assert (facts[10]["kc"], facts[10]["n_links"]) == (cc.SPEC_LABELS + 1, cc.FIN_LCAP) and facts[10]["g"] <= cc.FIN_GCAP
    assert routes == {"all_lanes": 1, "runs_lanes": 209, "runs_overflow": 0, "runs_rows": 0, "units_rows": 0, "runs_wave": 0, "runs_wave_scratch": 0,
                      "tail_narrow": 11, "tail_lds": 0, "tail_scratch": 0, "cap_tail": 64}
    assert on_host == 2


def test_mixed_case():
    facts, routes, on_host = analyse("mixed")
    assert sorted(set(_ms(facts))) == [cc.LANES_CAP, cc.LANES_CAP + 1, cc.CWR_CAP, cc.CWR_CAP + 1, 300]
    runs = [f["runs"] for f in facts]
    assert set(runs[:10]) == {1, 3, 4, 5, 8, 9, 15, 16, 17, 21}
    assert any(f["runs"] >= 60 and f["m"] <= cc.LANES_CAP for f in facts) and any(f["runs"] >= 60 and f["m"] > cc.CWR_CAP for f in facts)      # past 53 runs the double key rounds
    rows = [f["runs"] for f in facts[:10] if cc.LANES_CAP < f["m"] <= cc.CWR_CAP]
    assert sorted(r % cc.ROW_UNIT for r in rows) == [0, 0, 1, 3]      # whole units, 8 + 1, and a unit of fewer than 8
    # the windows one run alone decides: which run, among how many, in which run kernel, and what the key must not do (asserted in analyse)
    sole = [(f["m"], f["runs"], c["claims"]["key_variants"]) for f, c in zip(facts, cc.get("mixed")["contigs"]) if "key_variants" in c["claims"]]
    assert sole == [(64, 17, [{"omit": 16}]), (65, 21, [{"omit": 20}]), (255, 21, [{"omit": 16}]), (64, 60, [{"omit": 55}]), (256, 62, [{"omit": 57}]),
                    (64, 60, [{"exact": True}]), (256, 62, [{"exact": True}])]
    assert routes == {"all_lanes": 0, "runs_lanes": 155, "runs_overflow": 0, "runs_rows": 78, "units_rows": 12, "runs_wave": 169, "runs_wave_scratch": 0,
                      "tail_narrow": 5, "tail_lds": 12, "tail_scratch": 0, "cap_tail": 320}
    assert on_host == 0


def test_tables_case():
    facts, routes, on_host = analyse("tables")
    assert min(_ms(facts)) > cc.LANES_CAP and max(_ms(facts)) <= cc.CWR_CAP
    kgl = [(f["kc"], f["g"], f["n_links"], f["on_host"]) for f in facts]
    assert kgl[0] == (cc.FIN_KCAP, 8, 0, False) and kgl[1][0] == cc.FIN_KCAP + 1 and kgl[1][3]
    assert kgl[2] == (8, cc.FIN_GCAP, 0, False) and kgl[3] == (9, cc.FIN_GCAP + 1, 0, True)
    assert kgl[4][1:] == (5, cc.FIN_LCAP, False) and kgl[5][1:] == (5, cc.FIN_LCAP + 2, True)      # (g <= FIN_GCAP on both sides: the links alone decide)
    assert any(f["n_merged"] > 0 and not f["on_host"] for f in facts) and any(f["n_vetoed"] > 0 and not f["on_host"] for f in facts)
    assert routes == {"all_lanes": 0, "runs_lanes": 0, "runs_overflow": 0, "runs_rows": 258, "units_rows": 33, "runs_wave": 0, "runs_wave_scratch": 0,
                      "tail_narrow": 0, "tail_lds": 8, "tail_scratch": 0, "cap_tail": 192}
    assert on_host == 3


def test_alleles_case():
    facts, routes, on_host = analyse("alleles")
    assert _ms(facts) == [40, 64, 130, 256]
    assert routes == {"all_lanes": 0, "runs_lanes": 12, "runs_overflow": 4, "runs_rows": 6, "units_rows": 1, "runs_wave": 6, "runs_wave_scratch": 0,
                      "tail_narrow": 2, "tail_lds": 2, "tail_scratch": 0, "cap_tail": 256}
    assert on_host == 0


def test_columns_case():
    facts, routes, on_host = analyse("columns")
    assert max(_ms(facts)) <= cc.LANES_CAP
    cs = cc.get("columns")["contigs"]
    # the column of the walk that decides the window's link (asserted in analyse: without it the finished labels differ), among how many columns
    assert [(len(c["snp_pos"]), c["claims"]["split_variants"][0]["skip_col"]) for c in cs[1:7]] == \
        [(cc.TAIL_BATCH - 1, 6), (cc.TAIL_BATCH, 7), (cc.TAIL_BATCH + 1, 8), (2 * cc.TAIL_BATCH + 1, 16), (2 * cc.TAIL_BATCH + 1, 8), (2 * cc.TAIL_BATCH + 1, 7)]
    # the last entry of a column of 64 and of 65 that decides it
    assert [(c["claims"]["depths"][17], c["claims"]["split_variants"]) for c in cs[7:9]] == [(d, [{"cut_depth": d}]) for d in (cc.FAST_COLUMN, cc.FAST_COLUMN + 1)]
    assert set(np.diff(cs[7]["col_off"]).tolist()) == {cc.FAST_COLUMN} and np.diff(cs[8]["col_off"]).min() > cc.FAST_COLUMN      # batches without and with deep columns
    assert [c["claims"]["id_range"] for c in cs[9:11]] == [cc.TAIL_MAP_EXTRA, cc.TAIL_MAP_EXTRA + 1]
    assert sorted(set(cs[0]["claims"]["depths"].values())) == [cc.FAST_COLUMN, cc.FAST_COLUMN + 1]
    # the pair rule from both sides: SNPs PAIR_GAP apart and `> 9`, PAIR_GAP + 1 apart and `> 11`
    assert [(c["claims"]["gap_pairs"], c["claims"]["split_variants"]) for c in cs[12:14]] == [([(2, 3, False)], [{"gap": 9}]), ([(2, 3, True)], [{"gap": 11}])]
    assert facts[12]["n_merged"] == 1      # the register tail applies a link
    assert all(f["g"] >= 2 for f in facts)      # merge_wrongly_split_haplotypes walks the columns of every window
    assert routes == {"all_lanes": 1, "runs_lanes": 168, "runs_overflow": 0, "runs_rows": 0, "units_rows": 0, "runs_wave": 0, "runs_wave_scratch": 0,
                      "tail_narrow": 14, "tail_lds": 0, "tail_scratch": 0, "cap_tail": 64}
    assert on_host == 0


def test_scratch_cases():
    facts, routes, on_host = analyse("scratch")
    assert _ms(facts) == [cc.TAIL_LDS_NODES, cc.TAIL_LDS_NODES + 1] == [2048, 2049] and [f["runs"] for f in facts] == [5, 5]
    assert all(f["g"] >= 2 for f in facts)
    assert routes == {"all_lanes": 0, "runs_lanes": 0, "runs_overflow": 0, "runs_rows": 0, "units_rows": 0, "runs_wave": 10, "runs_wave_scratch": 0,
                      "tail_narrow": 0, "tail_lds": 1, "tail_scratch": 1, "cap_tail": 2048}
    assert on_host == 0
    facts, routes, on_host = analyse("scratch_alone")
    assert _ms(facts) == [cc.TAIL_LDS_NODES]
    assert (routes["tail_lds"], routes["tail_scratch"], routes["cap_tail"], routes["runs_wave"], on_host) == (1, 0, 2048, 5, 0)


def test_expected_routes_restates_the_lists():
    """expected_routes on made-up windows: every threshold from both sides"""
    f = lambda m, runs: {"m": m, "runs": runs}
    r = cc.expected_routes([f(64, 3), f(65, 9), f(255, 8), f(256, 2), f(12288, 1), f(12289, 1), f(10, 0)], [[16, 17, 18], [99] * 9, [1] * 8, [1, 1], [1], [1], []])
    assert r == {"all_lanes": 0, "runs_lanes": 3, "runs_overflow": 2, "runs_rows": 17, "units_rows": 3, "runs_wave": 4, "runs_wave_scratch": 1, "tail_narrow": 1,
                 "tail_lds": 3, "tail_scratch": 2, "cap_tail": 2048}
