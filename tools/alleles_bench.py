"""The allele table (HS_PIPELINE_ALLELES, hs_kernels_alleles.hip) on a job of a bench configuration, three ways, `steps` fused pipeline steps each after a
warm-up, sparse labels as bench.py takes them:
  1. ms per step with the option off and with HS_PIPELINE_ALLELES on (alternating blocks of steps on one pipeline);
  2. ms per step of the route a caller has without it: HS_PIPELINE_KEEP_COLUMNS (the .col payload comes to the host) and the crossing in numpy
     (tests/allele_cases.rule_numpy, window by window), reported apart and together;
  3. the kernels' own time (HIP events around the plan's and the cells' launches, summed over the contig groups) and their algorithmic bytes:
     entries x 5 B in, cells x 12 B out.
Usage: python tools/alleles_bench.py [config=C4] [contigs=0: the configuration's own] [steps=20] [groups=8]      (prints one JSON line)"""
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
    import allele_cases as ac
    import test_gpu_alleles as tg
    from hairsplitter_amd import api
    api.require_gpu()
    pg = api.PipelineGroups(contigs, groups)
    pg.sparse_labels(True)
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
        pg.alleles(False); off += block(max(1, steps // 4))[0]
        pg.alleles(True); t, sr = block(max(1, steps // 4)); on += t
    table = sr["alleles"]
    waits0 = api.host_waits(); block(4); waits_on = (api.host_waits() - waits0) / 4
    pg.alleles(False)
    waits0 = api.host_waits(); block(4); waits_off = (api.host_waits() - waits0) / 4
    # the kernels' own time: one step with events
    api.kernel_stats_every(1)
    pg.alleles(True)
    own = []
    for _ in range(5):
        _, sr = block(1)
        own.append(sr["alleles"]["t_kernel_ms"])
    api.kernel_stats_every(1 << 30)
    pg.alleles(False)
    # today's route: the columns on the host, the crossing in numpy
    pg.sparse_labels(False)
    pg.keep_columns(True)
    keep, cross = [], []
    for i in range(max(2, steps // 4)):
        t0 = time.perf_counter()
        cv, sr = pg.run_fused(0.33, 0, rarest_strain_abundance=0.01)
        t1 = time.perf_counter()
        cols = tg._group_columns(pg, 0.01)
        n_reads = np.diff(pg.flat.contig_rec_off)
        for c, ctg in enumerate(cols):
            ctg.update(length=0, read_start=np.zeros(n_reads[c], np.int32), read_end=np.zeros(n_reads[c], np.int32))
        host = ac.rule_numpy(cols, sr)
        t2 = time.perf_counter()
        if i:
            keep.append((t1 - t0) * 1e3); cross.append((t2 - t1) * 1e3)
    same = ac.differences(host, table) == []
    pg.close()
    med = statistics.median
    entries, cells = int(table["n_entries"]), int(len(table["cells"]))
    k_ms = med(own)
    print(json.dumps({
        "config": cfg, "contigs": n, "groups": groups, "steps": len(on),
        "ms_per_step_option_off": round(med(off), 3), "ms_per_step_alleles": round(med(on), 3),
        "ms_per_step_keep_columns": round(med(keep), 3), "ms_numpy_crossing_on_host": round(med(cross), 3),
        "ms_per_step_host_route": round(med(keep) + med(cross), 3),
        "host_waits_per_step": {"option_off": waits_off, "alleles": waits_on},
        "kernels": {"ms_summed_over_groups": round(k_ms, 4), "entries": entries, "cells": cells, "bytes": entries * 5 + cells * 12,
                    "GB_per_s": round((entries * 5 + cells * 12) / (k_ms * 1e6), 1) if k_ms > 0 else None, "wide_columns": int(table["n_wide_columns"])},
        "windows": int(len(table["win_start"])), "snps": int(len(table["snp_pos"])), "snps_separating_groups": int((table["snp_n_calls"] >= 2).sum()),
        "device_table_equals_numpy": bool(same)}))


if __name__ == "__main__":
    main()
