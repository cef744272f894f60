"""The comparison of a stage-4 call made through hs_sr_run_taps (chain mode) with the oracle's separate_reads_on_contig, both with their test taps on: used
by tests/test_gpu_kernels.py::test_clustering_chain_kernels_match_oracle (inputs that stage 3 made) and tests/test_gpu_chain_routes.py (inputs given directly)."""
import numpy as np


def compare_chain_with_oracle(out, contigs, oracle_taps):
    """out: the result dict of the call with out["taps"]; contigs: the per-contig inputs; oracle_taps: per contig, oracle_lib.sr_contig_taps on the same
    inputs. Asserts, for every contig: the finished labels of every window (exact); for every window with seeding SNPs the same reads, the same seeding
    SNPs, the labels of every per-SNP run (exact), and the third run as the same partition of the window's reads. -> (windows, runs) compared"""
    tp = out["taps"]
    n_runs = n_win = 0
    for c, ctg in enumerate(contigs):
        o = oracle_taps[c]
        N = len(ctg["read_start"])
        # the finished labels of every window of the contig
        w0, w1 = int(out["win_off"][c]), int(out["win_off"][c + 1])
        assert w1 - w0 == len(o["win_start"])
        for k in range(w1 - w0):
            assert int(out["win_start"][w0 + k]) == int(o["win_start"][k]) and int(out["win_end"][w0 + k]) == int(o["win_end"][k])
            got = out["labels"][int(out["label_off"][w0 + k]):int(out["label_off"][w0 + k + 1])]
            assert np.array_equal(got, o["win_labels"][k]), (c, k)
        # the chain's windows of this contig, in order: those of the oracle that have runs
        mine = np.flatnonzero(tp["win_contig"] == c)
        theirs = [k for k in range(len(o["tap_start"])) if o["run_begin"][k + 1] > o["run_begin"][k]]
        assert [int(tp["win_start"][k]) for k in mine] == [int(o["tap_start"][k]) for k in theirs]
        o_lab_off = 0
        o_off = {}
        for k in range(len(o["tap_start"])):
            m = int(o["tap_row0"][k + 1] - o["tap_row0"][k])
            o_off[k] = o_lab_off
            o_lab_off += m * int(o["run_begin"][k + 1] - o["run_begin"][k])
        for km, ko in zip(mine, theirs):
            ids = tp["mask_ids"][int(tp["win_row0"][km]):int(tp["win_row0"][km + 1])]
            oid = o["mask_ids"][int(o["tap_row0"][ko]):int(o["tap_row0"][ko + 1])]
            assert np.array_equal(ids, oid)
            m = len(ids)
            r0, r1 = int(tp["run_begin"][km]), int(tp["run_begin"][km + 1])
            assert np.array_equal(tp["run_snp"][r0:r1], o["run_snp"][int(o["run_begin"][ko]):int(o["run_begin"][ko + 1])])
            for i in range(r0, r1):
                got = tp["run_labels"][int(tp["run_off"][i]):int(tp["run_off"][i]) + m]
                exp = o["run_labels"][o_off[ko] + (i - r0) * m:o_off[ko] + (i - r0 + 1) * m]
                assert np.array_equal(got, exp), (c, int(tp["win_start"][km]), i - r0)
                n_runs += 1
            # the third run: the same partition of the window's reads (the oracle numbers the clusters by first appearance before it goes on, :972-981)
            g3 = tp["third"][int(tp["win_row0"][km]):int(tp["win_row0"][km + 1])]
            e3 = o["third"][int(o["tap_row0"][ko]):int(o["tap_row0"][ko + 1])]
            assert np.array_equal(g3 < 0, e3 < 0)
            pairs = set(zip(g3[g3 >= 0].tolist(), e3[e3 >= 0].tolist()))
            assert len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs)), (c, int(tp["win_start"][km]))
            n_win += 1
        assert N >= 0
    return n_win, n_runs
