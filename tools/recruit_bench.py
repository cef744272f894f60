"""The recruit table (HS_PIPELINE_RECRUIT, hs_kernels_recruit.hip) on a job of a bench configuration, `steps` fused pipeline steps each after a warm-up,
sparse labels as bench.py takes them:
  1. ms per step with HS_PIPELINE_ALLELES alone and with HS_PIPELINE_RECRUIT on top (alternating blocks of steps on one pipeline), and the host waits of both;
  2. the new kernels' own time (HIP events around the mark / scan and the count / decide launches, summed over the contig groups), rows, counter words and
     algorithmic bytes: per entry 4 B (mark) + 5 B (count), per label slot 8 B of fills, 16 B read and 16 B written by the two scans and 4 B read by
     the decide pass, per counter word 4 B filled + 4 B added + 4 B read, per row 40 B written;
  3. the route a caller has without it: HS_PIPELINE_KEEP_COLUMNS with HS_PIPELINE_ALLELES and the crossing in numpy (tests/recruit_cases.recruit_numpy);
  4. what the rule yields at the default thresholds, with HS_RECRUIT_LABELLED switched on as well for the evaluation rows: unlabelled rows per labelled
     row, the share of unlabelled rows assigned, and among the labelled rows the rule assigns the share whose best group is their own label.
Usage: python tools/recruit_bench.py [config=C4] [contigs=0: the configuration's own] [steps=20] [groups=8]      (prints one JSON line)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OWN = {"C2": 256, "C3": 50, "C4": 500, "C5": 34}


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "C4"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    groups = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    n = n or OWN.get(cfg, 50)
    import numpy as np
    from hairsplitter_amd import synth
    contigs, _ = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1))      # before the GPU is touched (forks)
    import recruit_cases as rc
    import test_gpu_alleles as tg
    from hairsplitter_amd import api
    api.require_gpu()
    pg = api.PipelineGroups(contigs, groups)
    pg.sparse_labels(True)
    pg.alleles(True)
    api.kernel_stats_every(1 << 30)      # timed steps record no events (bench.py times every 16th step only)

    def block(k):
        t = []
        for _ in range(k):
            t0 = time.perf_counter()
            cv, sr = pg.run_fused(0.33, 0, rarest_strain_abundance=0.01)
            t.append((time.perf_counter() - t0) * 1e3)
        return t, sr

    block(3)
    off, on = [], []
    for _ in range(4):      # alternating blocks: drift of the box hits both alike
        pg.recruits(False); off += block(max(1, steps // 4))[0]
        pg.recruits(True); t, sr = block(max(1, steps // 4)); on += t
    table = sr["recruits"]
    n_labels = int(sr["label_off"][-1])
    waits0 = api.host_waits(); block(4); waits_on = (api.host_waits() - waits0) / 4
    pg.recruits(False)
    waits0 = api.host_waits(); block(4); waits_off = (api.host_waits() - waits0) / 4
    # the kernels' own time: steps with events
    api.kernel_stats_every(1)
    pg.recruits(True)
    own, own_alleles = [], []
    for _ in range(5):
        _, sr = block(1)
        own.append(sr["recruits"]["t_kernel_ms"]); own_alleles.append(sr["alleles"]["t_kernel_ms"])
    # what the rule yields: the evaluation rows switched on as well
    pg.recruits(True, rc.params(which=rc.ABSENT | rc.UNCLUSTERED | rc.LABELLED))
    _, sr = block(1)
    r = sr["recruits"]["rows"]
    loose, lab = r[r["label"] < 0], r[r["label"] >= 0]
    lab_assigned = lab[lab["assigned"] != 0]
    yields = {"rows_absent": int((r["label"] == -2).sum()), "rows_unclustered": int((r["label"] == -1).sum()), "rows_labelled": int(len(lab)),
              "unlabelled_rows_per_labelled_row": round(len(loose) / max(len(lab), 1), 4),
              "share_of_unlabelled_rows_assigned": round(float((loose["assigned"] != 0).mean()) if len(loose) else 0.0, 4),
              "share_of_labelled_rows_assigned": round(len(lab_assigned) / max(len(lab), 1), 4),
              "concordance_of_assigned_labelled_rows": round(float((lab_assigned["best_group"] == lab_assigned["label"]).mean()) if len(lab_assigned) else 0.0, 4)}
    pg.recruits(False, rc.params())
    api.kernel_stats_every(1 << 30)
    # today's route: the columns on the host, the crossing in numpy (the cells from the allele table of the call)
    pg.sparse_labels(False)
    pg.keep_columns(True)
    keep, cross = [], []
    host = None
    for i in range(2):
        t0 = time.perf_counter()
        cv, sr = pg.run_fused(0.33, 0, rarest_strain_abundance=0.01)
        t1 = time.perf_counter()
        cols = tg._group_columns(pg, 0.01)
        n_reads = np.diff(pg.flat.contig_rec_off)
        for c, ctg in enumerate(cols):
            ctg.update(length=0, read_start=np.zeros(n_reads[c], np.int32), read_end=np.zeros(n_reads[c], np.int32))
        host = rc.recruit_numpy(cols, sr, rc.DEFAULT, alleles=sr["alleles"])
        t2 = time.perf_counter()
        if i:
            keep.append((t1 - t0) * 1e3); cross.append((t2 - t1) * 1e3)
    same = rc.differences(host, table) == []
    pg.close()
    med = statistics.median
    entries, rows, words = int(table["n_entries"]), int(len(table["rows"])), int(table["n_counter_words"])
    nbytes = 9 * entries + 44 * n_labels + 12 * words + 40 * rows
    k_ms = med(own)
    print(json.dumps({
        "config": cfg, "contigs": n, "groups": groups, "steps": len(on),
        "ms_per_step_alleles_only": round(med(off), 3), "ms_per_step_alleles_and_recruit": round(med(on), 3),
        "ms_per_step_keep_columns_and_alleles": round(med(keep), 3), "ms_numpy_crossing_on_host": round(med(cross), 3),
        "host_waits_per_step": {"alleles_only": waits_off, "alleles_and_recruit": waits_on},
        "kernels": {"ms_summed_over_groups": round(k_ms, 4), "ms_allele_kernels": round(med(own_alleles), 4), "entries": entries, "label_slots": n_labels, "rows": rows,
                    "counter_words": words, "bytes": nbytes, "GB_per_s": round(nbytes / (k_ms * 1e6), 1) if k_ms > 0 else None,
                    "share_of_8_TB_per_s": round(nbytes / (k_ms * 1e6) / 8000, 4) if k_ms > 0 else None},
        "windows": int(len(table["win_start"])), "rows_assigned": int(table["n_assigned"]), "yield_at_default_thresholds": yields,
        "device_table_equals_numpy": bool(same)}))


if __name__ == "__main__":
    main()
