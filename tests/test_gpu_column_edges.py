"""The column pass of stage 3 at its edges: the depth limit of a batch, contig ranges cut the way the pipeline's groups cut them, and the
automatic-SNP threshold away from 0.33 (float against double rounding of call_variants.cpp:531, the SNP merge of :1335-1352 at 0 and 1)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_kernels import (_check_candidate_bit_sets, _check_candidates, _check_leading_codes, _check_selection_and_gather,
                              _m_only_contig)

pytestmark = pytest.mark.gpu


def _one_position_contig(bases):
    """a contig of one base and one M-only one-base record per entry of `bases` (the codes at the position follow the read base)"""
    from hairsplitter_amd import synth
    n = len(bases)
    cig = np.array([(1 << 4) | synth.OP_M], np.uint32)
    alns = [synth.Alignment(k, 0, True, cig, 0) for k in range(n)]
    reads = list(np.asarray(bases, np.uint8).reshape(n, 1))
    return synth.ContigData("one", np.zeros(1, np.uint8), reads, [f"r{k}" for k in range(n)], alns, np.zeros(n, np.int32))


def test_depth_limit_of_a_batch(built):
    """hs_cv_batch_create refuses a position covered by more than 65535 records (K2 counts in 16-bit lanes, hs_cv_backend.inc) with
    HS_EINVAL; 65535 records over one position are accepted, and K2's counts and the column pass's leading codes there are the oracle's"""
    from hairsplitter_amd import api
    rng = np.random.default_rng(5)
    with pytest.raises(api.HsError, match=r"error -2: .*more than 65535 alignment records"):
        api.CvBatch(api.FlatBatch([_one_position_contig(rng.integers(0, 2, 65_536))]))
    for split in ((40_000, 25_535), (30_000, 30_000, 5_535)):
        bases = np.repeat(np.arange(len(split)), split)
        rng.shuffle(bases)
        flat = api.FlatBatch([_one_position_contig(bases)])
        t = api.device_tensors(flat)
        pile, _ = api.pileup(t, flat)
        st = api.column_stats(t, flat, pile)
        hp = pile.cpu().numpy()
        k0, k1, c0, c1, c2, depth = ol.column_top3(flat, hp, 0)
        assert int(depth[0]) == 65_535 and int(c0[0]) == split[0] and int(c1[0]) == split[1]
        assert int(st["depth"][0]) == 65_535
        assert st["cnt"][0, :3].astype(np.int32).tolist() == [int(c0[0]), int(c1[0]), int(c2[0])]
        b = api.CvBatch(flat)
        tp = api.cv_column_pass_taps(b, 0, 1, 0.33)
        b.close()
        _, _, md = ol.pileup(flat)
        assert len(tp["col_gpos"]) == 1
        _check_selection_and_gather(flat, tp, hp, md, 0, 1)
        _check_leading_codes(flat, tp, hp, 0, 1)
        _check_candidates(flat, tp, hp, md, 0, 1)


def _range_contigs():
    """normal contigs with tiny ones (1, 255, 256, 257 bases, each with reads) between them: the contig boundaries fall at offsets
    0, 1 and 255 of K2's 256-position tiles"""
    from hairsplitter_amd import synth
    # the one-base contig: records 1I1M whose inserted base (the previous base of the code at position 0) is A x 12, C x 6, T x 1: a column loop D reads
    ins = np.repeat(np.array([0, 1, 3], np.uint8), (12, 6, 1))
    cig = np.array([(1 << 4) | synth.OP_I, (1 << 4) | synth.OP_M], np.uint32)
    t1 = synth.ContigData("t1", np.array([2], np.uint8), [np.array([x, 2], np.uint8) for x in ins], [f"t1_r{k}" for k in range(len(ins))],
                          [synth.Alignment(k, 0, True, cig, 0) for k in range(len(ins))], np.zeros(len(ins), np.int32))
    cs = [synth.make_contig(31, 0, 2_560, 2, 0.01, 30, "ont", read_len_override=(300, 2000)), t1,
          synth.make_contig(31, 2, 255, 2, 0.02, 40, "ont", read_len_override=(60, 255)),
          synth.make_contig(31, 3, 256, 2, 0.02, 40, "ont", read_len_override=(60, 256)),
          synth.make_contig(31, 4, 2_815, 3, 0.01, 30, "ont", read_len_override=(300, 2000)),
          synth.make_contig(31, 5, 257, 2, 0.02, 40, "ont", read_len_override=(60, 257)),
          synth.make_contig(31, 6, 3_001, 2, 0.01, 30, "ont", read_len_override=(300, 2000))]
    return cs


def test_column_pass_on_contig_ranges_equals_whole_batch(built):
    """hs_cv_column_pass_taps over consecutive contig ranges, each on a fresh batch as a pipeline group starts (its own share of the
    pileup, K2 clipped to the range inside tiles it shares with its neighbour, the gathers and the candidate scan on the range's tiles):
    every range passes the checks against the oracle, and the ranges together are the whole batch's pass"""
    from hairsplitter_amd import api
    contigs = _range_contigs()
    flat = api.FlatBatch(contigs)
    offs = (flat.contig_off[1:-1] & 255).tolist()
    assert {0, 1, 255} <= set(offs), offs
    hp, _, md = ol.pileup(flat)
    b = api.CvBatch(flat)
    whole = api.cv_column_pass_taps(b, 0, flat.n_contigs, 0.33)
    b.close()
    assert len(whole["cand_col"]) > 0 and all(np.any(whole["col_rec"]["contig"] == c) for c in (1, 2, 3, 5))
    C = flat.n_contigs
    for cuts in ((1,), (2, 5), (1, 2, 4), (3, 4, 6), (1, 3, 5)):
        bounds = [0, *cuts, C]
        parts = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            b = api.CvBatch(flat)
            tp = api.cv_column_pass_taps(b, lo, hi, 0.33)
            b.close()
            _check_selection_and_gather(flat, tp, hp, md, lo, hi)
            _check_leading_codes(flat, tp, hp, lo, hi)
            _check_candidates(flat, tp, hp, md, lo, hi)
            _check_candidate_bit_sets(flat, tp)
            parts.append(tp)
        cat = lambda k: np.concatenate([p[k] for p in parts])
        assert np.array_equal(cat("col_gpos"), whole["col_gpos"]), cuts
        assert np.array_equal(cat("col_rec").view(np.uint8), whole["col_rec"].view(np.uint8)), cuts
        assert np.array_equal(cat("col_idx"), whole["col_idx"]) and np.array_equal(cat("col_code"), whole["col_code"]), cuts
        n_cols = np.cumsum([0] + [len(p["col_gpos"]) for p in parts])
        n_ent = np.cumsum([0] + [int(p["col_off"][-1]) for p in parts])
        assert np.array_equal(np.concatenate([p["col_off"][:-1] + n_ent[i] for i, p in enumerate(parts)] + [[n_ent[-1]]]), whole["col_off"]), cuts
        assert np.array_equal(np.concatenate([p["cand_col"] + n_cols[i] for i, p in enumerate(parts)]), whole["cand_col"]), cuts
        assert np.array_equal(cat("cand_rec").view(np.uint8), whole["cand_rec"].view(np.uint8)), cuts
        assert np.array_equal(cat("contig_n_cand"), whole["contig_n_cand"]) and np.array_equal(cat("contig_mean_distance"), whole["contig_mean_distance"])
        fields = [f for f in whole["cand_bits"].dtype.names if f != "word_off"]
        bits = cat("cand_bits")
        for f in fields:
            assert np.array_equal(bits[f], whole["cand_bits"][f]), (cuts, f)
        k = 0
        for p in parts:      # the bit-set blocks hold the same words (each pass numbers its own blocks)
            for h in p["cand_bits"]:
                hw = whole["cand_bits"][k]
                m = int(h["n_words"]) * (int(h["n_slots"]) + 1) + (int(h["n_slots"]) + 7) // 8
                assert np.array_equal(p["cand_words"][int(h["word_off"]):int(h["word_off"]) + m],
                                      whole["cand_words"][int(hw["word_off"]):int(hw["word_off"]) + m]), (cuts, k)
                k += 1
        assert k == len(whole["cand_bits"])


# second count : first count of the candidate columns of the threshold batch. At 0.35 and 0.7 the threshold's product rounds to the
# second count in float (0.35f * 20 == 7.0f, 0.7f * 10 == 7.0f) and lies below it in double: only the float comparison of
# call_variants.cpp:531 leaves these columns out of the automatic ones.
_RATIOS = ((5, 20), (7, 20), (5, 10), (7, 10), (9, 20))


def _thr_contigs():
    """one low-error contig per ratio: c1 reads carry the alternative base at 30 positions (one haplotype: loop C keeps those columns),
    then six positions where random sets of 4 other reads do (candidates that loops C and D do not keep, behind the last kept column)"""
    rng = np.random.default_rng(77)
    out = []
    for c1, c0 in _RATIOS:
        n = c0 + c1
        seq = rng.integers(0, 4, 1500).astype(np.uint8)
        M = np.tile(seq, (n, 1))
        hap = rng.choice(n, c1, replace=False)
        for i in range(30):
            p = 30 + 25 * i
            M[hap, p] = (seq[p] + 1) & 3
        rest = np.setdiff1d(np.arange(n), hap)
        for j in range(6):
            p = 1000 + 40 * j
            M[rng.choice(rest, 4, replace=False), p] = (seq[p] + 1) & 3
        out.append(_m_only_contig(f"r{c1}_{c0}", seq, [0] * n, list(M)))
    return out


def _oracle_call_variants(built, contigs, thr):
    from hairsplitter_amd import synth, canon
    with tempfile.TemporaryDirectory() as td:
        f = synth.write_files(contigs, td)
        col, vcf, err = (os.path.join(td, x) for x in ("o.col", "o.vcf", "o.err"))
        subprocess.run([built["oracle"], "call_variants", f["gfa"], f["reads"], f["sam"], "1", td, err, "0", "0", col, vcf, repr(float(thr))],
                       check=True, stdout=subprocess.DEVNULL)
        return canon.split_blocks(col), open(err).read()


def _assert_stage3_equals(out, contigs, blocks, o_err):
    """hs_cv_run's result against the oracle's .col / error rate, as test_stage3_result_equals_oracle_pipeline compares them"""
    assert "%g" % np.float32(out["error_rate"]) == o_err.strip()
    n_checked = 0
    for c, cd in enumerate(contigs):
        lines = blocks[cd.name]
        head = lines[0].split("\t")
        assert int(head[2]) == len(cd.seq)
        assert "%g" % np.float32(out["depth"][c]) == head[3]
        snps = [l.split("\t") for l in lines if l.startswith("SNPS")]
        s0, s1 = int(out["snp_off"][c]), int(out["snp_off"][c + 1])
        assert s1 - s0 == len(snps), cd.name
        for k, fld in enumerate(snps):
            s = s0 + k
            assert int(fld[1]) == int(out["snp_pos"][s]) and int(fld[2]) == int(out["snp_ref"][s]) and int(fld[3]) == int(out["snp_alt"][s])
            e0, e1 = int(out["col_off"][s]), int(out["col_off"][s + 1])
            assert [int(x) for x in fld[4].split(",") if x] == out["col_idx"][e0:e1].tolist()
            assert [int(x) for x in fld[5].split(",") if x] == out["col_code"][e0:e1].tolist()
            n_checked += 1
    assert n_checked == len(out["snp_pos"])


def test_automatic_snp_threshold(built):
    """HS_COL_AUTO of k_candidates_scan (`(float)c1 > thr * (float)c0` in float, call_variants.cpp:531) at thresholds where float and double
    disagree, and the SNP list of hs_cv_run -- the automatic and the kept columns merged until either list ends (:1335-1352) -- at 0
    (every candidate is automatic: the list stops at the last kept column), 0.35 and 1 (nothing is automatic: no SNP at all)"""
    from hairsplitter_amd import api
    contigs = _thr_contigs()
    flat = api.FlatBatch(contigs)
    hp, _, md = ol.pileup(flat)
    assert np.all(md.astype(np.float64) < 0.015)
    f32 = np.float32
    for thr, (c1, c0) in ((0.35, (7, 20)), (0.7, (7, 10))):      # the regime: float and double disagree on these columns
        assert f32(thr) * f32(c0) == f32(c1) and float(f32(thr)) * c0 < c1
    n_auto = {}
    for thr in (0.0, 0.25, 0.35, 0.5, 0.7, 1.0):
        b = api.CvBatch(flat)
        tp = api.cv_column_pass_taps(b, 0, flat.n_contigs, thr)
        b.close()
        _check_candidates(flat, tp, hp, md, 0, flat.n_contigs, thr=thr)
        rec = tp["col_rec"]
        n_auto[thr] = {(int(a), int(b_)): int(((rec["flags"] & 2) != 0)[(rec["c1"] == a) & (rec["c0"] == b_)].sum()) for a, b_ in _RATIOS}
        assert all(int(((rec["flags"] & 1) != 0)[(rec["c1"] == a) & (rec["c0"] == b_)].sum()) >= 30 for a, b_ in _RATIOS)
    assert n_auto[0.35][(7, 20)] == 0 and n_auto[0.35][(9, 20)] > 0 and n_auto[0.25][(5, 20)] == 0 and n_auto[0.25][(7, 20)] > 0
    assert n_auto[0.7][(7, 10)] == 0 and n_auto[0.5][(5, 10)] == 0 and n_auto[0.5][(7, 10)] > 0 and n_auto[1.0] == {r: 0 for r in _RATIOS}
    # hs_cv_run at 0, 0.35 and 1 against the oracle's call_variants with the same threshold argument
    for thr in (0.0, 0.35, 1.0):
        b = api.CvBatch(flat)
        out = b.run(thr)
        b.close()
        blocks, o_err = _oracle_call_variants(built, contigs, thr)
        _assert_stage3_equals(out, contigs, blocks, o_err)
        if thr == 1.0:
            assert int(out["snp_off"][-1]) == 0
        if thr == 0.0:      # every candidate is automatic; the list is cut where the kept list ends: here one contig keeps none
            n_snp = np.diff(out["snp_off"])
            n_aut = np.array([int((ol.call_variants_flags(flat, hp, c, float(md[c]), automatic_snp_threshold=0.0) & 2).astype(bool).sum())
                              for c in range(flat.n_contigs)])
            assert np.all(n_aut >= 30) and np.any(n_snp == 0) and np.any(n_snp > 0)
    # the pipeline's size hints of one step must not leak into the next, whose SNP set differs
    groups = api.PipelineGroups(contigs, 3)
    try:
        for thr in (1.0, 0.0, 1.0):
            single = api.CvBatch(api.FlatBatch(contigs))
            cv1, sr1 = single.run_pipeline(thr, 8)
            single.close()
            cv3, sr3 = groups.run_fused(thr, 8)
            assert np.array_equal(cv1["mean_distance"], cv3["mean_distance"])
            assert np.float32(min(float("%g" % cv1["error_rate"]), 0.15)) == np.float32(cv3["error_rate"])
            assert cv1["n_snps"] == cv3["n_snps"] and (cv3["n_snps"] == 0) == (thr == 1.0), thr
            assert np.array_equal(sr1["win_off"], sr3["win_off"]) and np.array_equal(sr1["label_off"], sr3["label_off"])
            assert np.array_equal(sr1["labels"], sr3["labels"])
            assert np.array_equal(sr1["win_start"], sr3["win_start"]) and np.array_equal(sr1["win_end"], sr3["win_end"])
    finally:
        groups.close()
