"""The front of stage 4 in the layout hs_sr_run launches it in: K5a k_snp_planes, K5 k_simdiff, k_simdiff_windows, K6 k_read_graph_rows<false / true> and
the row fetch, patch, degree and fill kernels, reached through hs_sr_run_taps in its graphs mode (hs::sr_run's own calls of simdiff_columns,
build_graphs_begin / _end and fetch_graphs: es = 2 pairs, rows by start position, word ranges from K5a, skipped tiles, several contigs in one plane array,
matrix and low-memory windows in one row space). One test per case of tests/graph_cases.py (tests/test_cpu_graph_cases.py shows, without a GPU, that every
case is what its table says). Everything is compared for exact integer equality with the oracle:

  planes   bit (r, s) of alt / ref == (code == alt) / (code == ref), every word of every row (the buffers are all ones before K5a);
  sim/diff every entry on both sides of the diagonal == the oracle's list_similarities_and_differences mapped through pos_orig, or the sentinel the
           matrices are filled with before K5 -- and the sentinel only where the oracle has (0, 0) (a tile K5 skips);
  graphs   every window's mask == the oracle's separate_reads_on_contig mask, its neighbour lists == the oracle's create_read_graph_matrix /
           create_read_graph_low_memory on that mask; and the counters of the call show that the case went the way it was built to go.

Left out: a window of more than 7168 reads, the cap beyond which the row kernels hand every row of the window to the host -- its contig's matrices alone
are hundreds of MB."""
import numpy as np
import pytest

import graph_cases as gc
import oracle_lib as ol

pytestmark = pytest.mark.gpu
SENTINEL = -2 ** 31


def _run(name):
    from hairsplitter_amd import api
    assert api.SR_TAP_SENTINEL == SENTINEL
    case = gc.get(name)
    return case, api.separate_reads_graph_taps(case["contigs"], case["window"], case["error_rate"], low_memory=case["low_memory"])


def _check_planes(case, tp):
    """every contig with SNPs has bit rows: the matrix path reads them in K5, the low-memory path in k_simdiff_windows"""
    assert len(tp["words"]) == len(case["contigs"])
    total = 0
    for ci, c in enumerate(case["contigs"]):
        N, W = len(c["read_start"]), (len(c["snp_pos"]) + 63) // 64
        if W == 0:
            assert tp["words"][ci] == 0
            continue
        assert tp["words"][ci] == W and tp["plane_n"][ci] == N
        o = int(tp["plane_off"][ci])
        alt, ref = gc.expected_planes(c)
        assert np.array_equal(tp["alt"][o:o + N * W].reshape(N, W), alt), ("alt", ci)
        assert np.array_equal(tp["ref"][o:o + N * W].reshape(N, W), ref), ("ref", ci)
        total += N * W
    assert len(tp["alt"]) == total and len(tp["ref"]) == total


def _check_matrices(name, case, tp):
    """-> per matrix contig: (sentinel mask [N, N] in matrix order, pos_orig)"""
    out = {}
    total = 0
    for ci, c in enumerate(case["contigs"]):
        N = len(c["read_start"])
        lm = case["low_memory"] or gc.coverage_above_1000(c)
        if lm or len(c["snp_pos"]) == 0:
            assert tp["n_reads"][ci] == 0
            continue
        assert tp["n_reads"][ci] == N
        rb = int(tp["read_base"][ci])
        po = tp["pos_orig"][rb:rb + N]
        assert np.array_equal(po, gc.start_order(c)), ci
        o = int(tp["out_off"][ci])
        got = tp["matrix"][o:o + N * N].reshape(N, N, 2)
        sim, diff = gc.oracle_simdiff(ol, name, ci)
        want = np.stack((sim[np.ix_(po, po)], diff[np.ix_(po, po)]), axis=2)
        sent = np.all(got == SENTINEL, axis=2)
        assert np.array_equal(np.any(got == SENTINEL, axis=2), sent), ci                  # a pair is written whole or not at all
        assert np.array_equal(got[~sent], want[~sent]), ci
        assert not np.any(want[sent]), ci                                                 # the sentinel only where the oracle has (0, 0)
        out[ci] = (sent, po)
        total += N * N
    assert len(tp["matrix"]) == total
    return out


def _check_graphs(name, case, tp):
    """-> kinds of the windows, per contig"""
    masks = gc.oracle_masks(ol, name)
    W = len(tp["win_contig"])
    assert W == sum(len(x) for x in masks)
    assert np.all(np.diff(tp["win_kind"]) >= 0)      # matrix windows, low-memory windows of the device, then the host's
    seen = [0] * len(case["contigs"])
    kinds = [[] for _ in case["contigs"]]
    for w in range(W):
        ci, kind = int(tp["win_contig"][w]), int(tp["win_kind"][w])
        r0, r1 = int(tp["win_row0"][w]), int(tp["win_row0"][w + 1])
        ids = tp["mask_ids"][r0:r1]
        assert np.array_equal(ids, masks[ci][seen[ci]]), (ci, seen[ci])
        seen[ci] += 1
        lm = case["low_memory"] or gc.coverage_above_1000(case["contigs"][ci])
        assert (kind > 0) == lm, (ci, kind)
        kinds[ci].append(kind)
        got = [tp["nbr"][tp["nbr_off"][r]:tp["nbr_off"][r + 1]].tolist() for r in range(r0, r1)]
        want = gc.oracle_graph(ol, name, ci, ids, kind)
        for k in range(r1 - r0):
            assert got[k] == want[k], (name, "contig", ci, "window", seen[ci] - 1, "read", int(ids[k]))
    assert seen == [len(x) for x in masks]
    return kinds


def _check_all(name):
    case, tp = _run(name)
    _check_planes(case, tp)
    mats = _check_matrices(name, case, tp)
    kinds = _check_graphs(name, case, tp)
    return case, tp, mats, kinds


def test_blocks(built):
    """N in {1 .. 600} x S in {1 .. 1025}: K5a's second round of 512 reads, partial last word, fewer than 4 words; K5's diagonal and mirrored tiles,
    ragged N. Every read is in every column: no entry may be the sentinel."""
    case, tp, mats, _ = _check_all("blocks")
    assert len(mats) == len(case["contigs"])
    for sent, _ in mats.values():
        assert not sent.any()
    assert tp["row_waves"] == 4


def test_packed(built):
    """five contigs in one plane array, S = 70, 0, 256, 3, 130: a contig boundary inside a 256-column block of K5a, a contig without SNPs between others"""
    case, tp, mats, _ = _check_all("packed")
    assert sorted(mats) == [0, 2, 3, 4]
    assert tp["plane_off"][2] == 40 * 2 and tp["words"][1] == 0


def test_tiled(built):
    """400 short reads along 33 words, read index shuffled against start: orig_of / pos_rank, word ranges, w_begin rounding, w_end clamp, skipped tiles"""
    case, tp, mats, _ = _check_all("tiled")
    c = case["contigs"][0]
    sent, po = mats[0]
    nb = (len(po) + 63) // 64
    skipped = computed_late = 0
    for i in range(nb):
        for j in range(nb):
            tile = sent[64 * i:64 * i + 64, 64 * j:64 * j + 64]
            words = gc.tile_words(c, min(i, j), max(i, j))
            assert tile.all() == (words is None), (i, j)      # K5 skips exactly the tiles whose blocks share no word
            assert tile.all() or not tile.any(), (i, j)
            skipped += bool(tile.all())
            computed_late += bool(words is not None and words[0] > 0)
    assert skipped > 0 and computed_late > 0


def test_fringe(built):
    """ranges that begin and end at word 15 / 16 / 17, from presence alone (the first and the last SNP of a read carry a third allele)"""
    case, tp, mats, _ = _check_all("fringe")
    c = case["contigs"][0]
    sent, po = mats[0]
    for (i, j), words in (((0, 3), (0, 16)), ((0, 4), None), ((1, 4), (16, 17)), ((1, 5), None), ((2, 5), (16, 18))):
        assert gc.tile_words(c, i, j) == words
        for a, b in ((i, j), (j, i)):
            assert sent[64 * a:64 * a + 64, 64 * b:64 * b + 64].all() == (words is None), (a, b)


def test_ties(built):
    """S = 16 with 15 % noise: rows whose cut-off falls into a run of equal distances go to the host, more of them than a first call's staging area
    holds -- k_read_graph_fetch_rows on the (sim, diff) pairs, the host's pos_rank permutation, k_read_graph_patch"""
    case, tp, _, _ = _check_all("ties")
    assert tp["rows_on_host"] > 64 and 0 < tp["rows_late"] < tp["rows_on_host"]


def test_small_m(built):
    """windows of 0, 1, 2, 5, 6, 64 and 65 reads, a contig of one read: the five-neighbour cut, one and two words of link bits, the N < 2 give-up"""
    case, tp, _, _ = _check_all("small_m")
    assert sorted(np.diff(tp["win_row0"]).tolist()) == [0, 1, 1, 2, 5, 6, 64, 65]
    assert tp["rows_on_host"] >= 1      # the row of the one-read contig


def test_wide(built):
    """a window of 1800 reads: the row kernel's one-wave launch (more than 1792 distances per wavefront do not fit four to a workgroup)"""
    case, tp, _, _ = _check_all("wide")
    assert 1793 <= int(np.diff(tp["win_row0"]).max()) <= 1856
    assert tp["row_waves"] == 1


def test_lm_flag(built):
    """low_memory = 1: k_simdiff_windows and k_read_graph_rows<true> at m = 63, 64, 65, 130"""
    case, tp, mats, kinds = _check_all("lm_flag")
    assert not mats and len(tp["matrix"]) == 0
    assert [k for ks in kinds for k in ks] == [1, 1, 1, 1]
    assert tp["row_waves"] == 4


def test_lm_mixed(built):
    """a contig with coverage > 1000 between two matrix contigs: both kinds of device windows in one row space, bit rows of the low-memory contig in read order"""
    case, tp, mats, kinds = _check_all("lm_mixed")
    assert kinds == [[0], [1], [0]] and sorted(mats) == [0, 2]
    assert tp["plane_n"].tolist() == [50, 1040, 45] and tp["n_reads"].tolist() == [50, 0, 45]


def test_lm_nan(built):
    """masked pairs that share third alleles only: 0 / 0 distances, the rows go to the host"""
    case, tp, _, kinds = _check_all("lm_nan")
    assert all(k == [1] for k in kinds)
    assert tp["rows_on_host"] > 0


def test_lm_gap(built):
    """a read that skips a SNP inside its span: that contig's windows stay with the host builder, the other's are the device's; the graphs are the oracle's"""
    case, tp, _, kinds = _check_all("lm_gap")
    assert kinds == [[1], [2]]


def test_graph_taps_behind_stage_3(built):
    """api.separate_reads(taps="graphs") on what stage 3 made of a small synthetic contig: the same comparisons on columns the pipeline itself wrote"""
    from hairsplitter_amd import api, synth
    flat = api.FlatBatch([synth.make_contig(7, 0, 12_000, 2, 0.01, 30, "ont"), synth.make_contig(8, 1, 9_000, 3, 0.01, 40, "ont")])
    b = api.CvBatch(flat)
    cv = b.run(0.33)
    b.close()
    er = min(float("%g" % np.float32(cv["error_rate"])), 0.15)
    out = api.separate_reads(cv, flat, er, taps="graphs")
    case = {"contigs": out["contigs"], "window": out["window_size"], "error_rate": er, "low_memory": False}
    gc.register("stage3", case)
    tp = out["taps"]
    _check_planes(case, tp)
    mats = _check_matrices("stage3", case, tp)
    _check_graphs("stage3", case, tp)
    assert len(mats) > 0 and len(tp["win_contig"]) > 0
