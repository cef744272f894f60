"""The cases of tests/graph_cases.py are what their table says, and the graphs mode of the stage-4 test taps hands over what sr_run built: no GPU, the oracle
alone. tests/harness/host_harness graph_taps runs hs::sr_run on the oracle's device interface in the graphs mode of hs::SrTaps; its windows and neighbour
lists are compared, window by window, with the oracle's create_read_graph_matrix / create_read_graph_low_memory on the tapped mask, and its masks with the
oracle's separate_reads_on_contig."""
import os
import subprocess

import numpy as np
import pytest

import graph_cases as gc
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "_build", "host_harness")


@pytest.fixture(scope="module", autouse=True)
def _artefacts(built):
    return built


def test_low_memory_contigs_by_coverage():
    """only the middle contig of lm_mixed has coverage > 1000; `wide` keeps its 1824 reads on the matrix path"""
    for name in gc.CASES:
        got = [gc.coverage_above_1000(c) for c in gc.get(name)["contigs"]]
        assert got == ([False, True, False] if name == "lm_mixed" else [False] * len(got)), name
    c = gc.get("lm_mixed")["contigs"][1]
    assert 1000 < len(c["read_start"]) <= 1048


def test_blocks_shapes():
    cs = gc.get("blocks")["contigs"]
    assert {len(c["read_start"]) for c in cs} == {1, 2, 63, 64, 65, 511, 512, 513, 600}
    assert {len(c["snp_pos"]) for c in cs} == {1, 64, 65, 255, 256, 257, 1025}
    for c in cs:      # all reads span the contig: every read in every column
        assert np.all(np.diff(c["col_off"]) == len(c["read_start"]))


def test_packed_shapes():
    for name in ("packed", "lm_flag"):
        assert [len(c["snp_pos"]) for c in gc.get(name)["contigs"]] == [70, 0, 256, 3, 130]
    assert gc.get("lm_flag")["low_memory"] and not gc.get("packed")["low_memory"]


def test_tiled_block_ranges():
    """restated in numpy: rows in start order, 64 to a block, a block's words = first .. last word any of its reads is present in"""
    c = gc.get("tiled")["contigs"][0]
    N = len(c["read_start"])
    assert N == 400 and len(c["snp_pos"]) == 2100
    o = gc.start_order(c)
    assert not np.array_equal(o, np.arange(N))                                    # read index shuffled against start
    assert len(np.unique(c["read_start"])) < N // 4                              # many equal starts
    lo, hi = gc.presence_words(c)
    assert np.all(hi[o[:64]] < 0) and 0 < np.sum(hi[o[64:]] < 0) < 64            # one whole block in no column, and some reads elsewhere
    nb = (N + 63) // 64
    tiles = {(i, j): gc.tile_words(c, i, j) for i in range(nb) for j in range(i, nb)}
    assert any(t is None for (i, j), t in tiles.items() if i > 0)                # a pair of blocks (both with reads in columns) that shares no word
    assert any(t is not None and t[0] >= 16 for t in tiles.values())             # a pair that shares words from word 16 on only
    assert any(t is not None and t[1] < 33 for t in tiles.values())              # ... and one that stops before the last word


def test_fringe_block_ranges():
    c = gc.get("fringe")["contigs"][0]
    lo, hi = gc.block_word_ranges(c)
    assert lo.tolist() == [0, 0, 0, 15, 16, 17, 17] and hi.tolist() == [15, 16, 17, 32, 32, 32, 32]
    assert gc.tile_words(c, 0, 3) == (0, 16) and gc.tile_words(c, 0, 4) is None and gc.tile_words(c, 1, 4) == (16, 17) and gc.tile_words(c, 2, 5) == (16, 18)
    # the first and the last SNP of every read carry neither allele: the planes alone would give a narrower range
    alt, ref = gc.expected_planes(c)
    plo, phi = gc.presence_words(c)
    S = len(c["snp_pos"])
    seg = np.repeat(np.arange(S), np.diff(c["col_off"]))
    first = np.full(len(plo), S); last = np.full(len(plo), -1)
    np.minimum.at(first, c["col_idx"], seg); np.maximum.at(last, c["col_idx"], seg)
    both = alt | ref
    for r in range(len(plo)):
        for s in (int(first[r]), int(last[r])):
            assert not (int(both[r, s // 64]) >> (s % 64)) & 1


def test_lm_nan_has_pairs_without_common_allele():
    n = 0
    for ci, ids_list in enumerate(gc.oracle_masks(ol, "lm_nan")):
        sim, diff = gc.oracle_simdiff(ol, "lm_nan", ci)
        for ids in ids_list:
            sub = (sim + diff)[np.ix_(ids, ids)]
            n += int(np.sum(sub == 0)) - len(ids)
    assert n > 0


def test_lm_gap_breaks_the_run_of_presence():
    cs = gc.get("lm_gap")["contigs"]
    assert [gc.presence_is_one_run(c) for c in cs] == [True, False]
    r, s = cs[1]["gap"]
    assert r in gc.oracle_masks(ol, "lm_gap")[1][0]
    for name in gc.CASES:
        if name != "lm_gap":
            assert all(gc.presence_is_one_run(c) for c in gc.get(name)["contigs"]), name


def test_ties_has_more_ambiguous_rows_than_the_first_staging_area_holds():
    """a first call stages the rows of at most 64 undecided rows of the longest contig: more than 64 of them means rows fetched late"""
    case = gc.get("ties")
    n = 0
    for ci, ids_list in enumerate(gc.oracle_masks(ol, "ties")):
        sim, diff = gc.oracle_simdiff(ol, "ties", ci)
        n += sum(gc.ambiguous_rows(sim, diff, ids, case["error_rate"]) for ids in ids_list)
    assert n > 64


@pytest.mark.parametrize("name", list(gc.CASES))
def test_mask_sizes(name):
    masks = gc.oracle_masks(ol, name)
    for c, ids_list in zip(gc.get(name)["contigs"], masks):
        if c["mask_sizes"] is not None:
            assert [len(x) for x in ids_list] == c["mask_sizes"]
    sizes = sorted(len(x) for ids_list in masks for x in ids_list)
    if name == "small_m":
        assert sizes == [0, 1, 1, 2, 5, 6, 64, 65] and min(len(c["read_start"]) for c in gc.get(name)["contigs"]) == 1
    if name == "lm_flag":
        assert sizes == [63, 64, 65, 130]
    if name == "wide":
        assert len(sizes) == 1 and 1793 <= sizes[0] <= 1856
    if name in ("tiled", "fringe"):
        assert len(sizes) == 5 and max(sizes) > 64


@pytest.mark.parametrize("name", list(gc.CASES))
def test_graph_taps_on_the_oracle_interface(name, tmp_path):
    case = gc.get(name)
    fin, fout = str(tmp_path / "in.i64"), str(tmp_path / "out.i64")
    gc.to_i64(case).tofile(fin)
    subprocess.run([HARNESS, "graph_taps", fin, fout], check=True)
    on_host, wins = gc.from_i64(np.fromfile(fout, np.int64))
    masks = gc.oracle_masks(ol, name)
    assert len(wins) == sum(len(x) for x in masks)
    seen = [0] * len(case["contigs"])
    for w in wins:
        ci = w["contig"]
        lm = case["low_memory"] or gc.coverage_above_1000(case["contigs"][ci])
        assert w["kind"] == (2 if lm else 0)      # (the oracle's device interface leaves the low-memory path to the host builder)
        assert np.array_equal(w["ids"], masks[ci][seen[ci]]), (name, ci, seen[ci])
        seen[ci] += 1
        assert w["nbr"] == gc.oracle_graph(ol, name, ci, w["ids"], w["kind"]), (name, ci)
    assert seen == [len(x) for x in masks]
    assert [w["kind"] for w in wins] == sorted(w["kind"] for w in wins)      # matrix windows first
