"""The polisher's inputs (hs_polish_inputs: k_polish_cut, k_polish_gather) on a job of a bench configuration, with the labels of one
pipeline step: own time of the two kernels (HIP events around their launches), algorithmic bytes and the fraction of the HBM peak,
median of `runs` calls after a warm-up. Next to it, where oracle/_ref holds HS_create_new_contigs, the wall time of the reference's
stage 5 on the files of the same job with the stand-in executables of tools/record_polish_goldens.py (no polisher runs), on one
thread and on 16: its parsing and the .gaf are inside that time, the external tools are not.
Usage: python tools/polish_bench.py [config=C4] [contigs=0: the configuration's own] [runs=5]      (prints one JSON line)
       python tools/polish_bench.py consensus [config=C4] [contigs=60] [runs=5]
       python tools/polish_bench.py haplotypes [config=C4] [contigs=60] [runs=5] [alternations=3]
consensus: the consensus of the same job's bundles (hs_polish_consensus) -- per kernel group own time, algorithmic bytes and
the fraction of the HBM peak, the whole call, the host half on 16 threads on the same bundles, and how much of the backbones changed.
haplotypes: from the labels to the haplotype sequences -- the whole call of polish_haplotypes and of polish_inputs followed by
polish_consensus, alternating three times (median of `runs` calls after a warm-up each time); the own time of k_cons_plan + layout, its
algorithmic bytes and fraction of the HBM peak; what either route moved. A build without hs_polish_haplotypes times the composition alone.
       python tools/polish_bench.py refine [config=C4] [contigs=60] [runs=5] [alternations=3]
refine: polishing passes -- polish_haplotypes with 1, 2 and 3 passes, alternating (median of `runs` calls after a warm-up each time):
the whole call, per pass the time per phase, the waits and the change counters, what the call moved; the own time of k_refine_windows +
k_refine_gather with its algorithmic bytes and fraction of the HBM peak, and A1's share of a pass. A build without the passes times one pass alone."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E
OWN = {"C2": 256, "C3": 50, "C4": 500, "C5": 34}


def reference_wall(paths, files, gro, td, threads):
    import record_polish_goldens as rec
    tools, tmp = os.path.join(td, "standins"), os.path.join(td, "cnc_tmp_%d" % threads)
    os.makedirs(tools, exist_ok=True); os.makedirs(tmp)
    cap = os.path.join(td, "capture_%d" % threads)
    os.makedirs(cap)
    rec._script(os.path.join(tools, "minimap2"), rec.MINIMAP2)
    rec._script(os.path.join(tools, "samtools"), "#!/bin/sh\nexit 0\n")
    rec._script(os.path.join(tools, "racon"), "#!/bin/sh\nexit 1\n")
    env = dict(os.environ, HS_POLISH_CAPTURE=cap, PATH=tools + os.pathsep + os.environ.get("PATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run([paths["ref_cnc"], files["gfa"], files["reads"], "0.05", gro, files["sam"], tmp + "/", str(threads), "ont", os.path.join(tmp, "o.gfa"),
                        os.path.join(tmp, "o.gaf"), "racon", "0", "0", os.path.join(tools, "minimap2"), os.path.join(tools, "racon"), "/nonexistent/medaka",
                        os.path.join(tools, "samtools"), "/nonexistent/python", "0"], cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return {"threads": threads, "seconds": time.perf_counter() - t0, "exit_status": r.returncode, "bundles_handed_to_the_polisher": len(os.listdir(cap))}


def consensus_row_bytes(res):
    """one byte per piece and covered column: sum(M + D) of every piece that is not skipped, clipped at the end of its backbone"""
    import numpy as np
    w = res["cigar"].astype(np.int64)
    ln, op = w >> 4, w & 15
    at = res["cig_off"][:-1]

    def per_piece(x):
        c = np.concatenate(([0], np.cumsum(x)))
        return c[res["cig_off"][1:]] - c[at]
    cols, rd = per_piece(np.where((op == 0) | (op == 2), ln, 0)), per_piece(np.where((op == 0) | (op == 1), ln, 0))
    n_bases = np.diff(res["base_off"])
    L = np.repeat(np.diff(res["backbone_off"]), np.diff(res["piece_off"]))
    s0 = res["piece_sam_pos"].astype(np.int64) - 1
    ok = (n_bases > 0) & ((res["piece_flags"] & 2) == 0) & (rd == n_bases) & (s0 < L)
    return int(np.where(ok, np.minimum(cols, L - s0), 0).sum())


def main_consensus(argv):
    cfg = argv[0] if argv else "C4"
    n = int(argv[1]) if len(argv) > 1 else 60
    runs = max(5, int(argv[2])) if len(argv) > 2 else 5
    from hairsplitter_amd import synth
    with tempfile.TemporaryDirectory() as td:
        contigs, files = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1), outdir=td)      # before the GPU is touched (forks)
        from hairsplitter_amd import api
        api.require_gpu()
        pl = api.PipelineGroups(contigs, 4)
        cv, sr = pl.run_fused(0.33, 0, rarest_strain_abundance=0.01)
        res = api.polish_inputs(pl, sr)
        pl.close()
    samples = []
    for i in range(runs + 1):
        w0 = api.host_waits()
        t0 = time.perf_counter()
        cons = api.polish_consensus(res)
        wall = time.perf_counter() - t0
        if i:      # the first call is the warm-up
            samples.append((cons["stats"], wall, api.host_waits() - w0))
    st = cons["stats"]
    C, rb = int(res["backbone_off"][-1]), consensus_row_bytes(res)
    text = int(cons["cons_off"][-1])
    bytes_of = {"rows": 4 * int(res["cig_off"][-1]) + int(res["base_off"][-1]) + rb + 24 * st["n_ins_records"], "columns": rb + 6 * C + 32 * res["n_pieces"],
                "ins": 24 * st["n_ins_records"] + 5 * C, "emit": 22 * C + 2 * text}
    out = {"mode": "consensus", "config": cfg, "contigs": n, "runs": runs, "bundles": res["n_bundles"], "pieces": res["n_pieces"], "columns": C, "row_bytes": rb,
           "rounds": st["n_rounds"], "host_waits_per_call": samples[-1][2], "ins_records": st["n_ins_records"], "ins_slots": st["n_ins_slots"],
           "call_wall_ms_median": statistics.median(w for _, w, _ in samples) * 1e3,
           "changed": {k: int(cons[k].sum()) for k in ("n_sub", "n_del", "n_ins_bases", "n_low", "n_skipped")}, "consensus_bytes": text}
    for k in ("rows", "columns", "ins", "emit"):
        ms = statistics.median(s[k + "_ms"] for s, _, _ in samples)
        out["k_cons_" + k] = {"ms_median": ms, "algorithmic_bytes": bytes_of[k]}
        if ms > 0:
            gbs = bytes_of[k] / (ms * 1e-3) / 1e9
            out["k_cons_" + k].update({"GBs": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBS})
    os.environ["HS_CONSENSUS_HOST_THREADS"] = "16"
    host_wall = []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        host = api.polish_consensus(res, form="host")
        if i:
            host_wall.append(time.perf_counter() - t0)
    out["host_half_16_threads_ms_median"] = statistics.median(host_wall) * 1e3
    out["device_equals_host"] = bool(all((cons[k] == host[k]).all() for k in ("cons_off", "cons", "trim_start", "trim_end", "n_sub", "n_del", "n_ins_bases", "n_low", "n_skipped")))
    print(json.dumps(out))


def main_haplotypes(argv):
    cfg = argv[0] if argv else "C4"
    n = int(argv[1]) if len(argv) > 1 else 60
    runs = max(5, int(argv[2])) if len(argv) > 2 else 5
    alternations = int(argv[3]) if len(argv) > 3 else 3
    from hairsplitter_amd import synth
    with tempfile.TemporaryDirectory() as td:
        contigs, files = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1), outdir=td)      # before the GPU is touched (forks)
        from hairsplitter_amd import api
        api.require_gpu()
        pl = api.PipelineGroups(contigs, 4)
        cv, sr = pl.run_fused(0.33, 0, rarest_strain_abundance=0.01)
        have = hasattr(api, "polish_haplotypes")

        def composed():
            res = api.polish_inputs(pl, sr)
            return res, api.polish_consensus(res)

        def timed(call):
            walls, waits, last = [], [], None
            for i in range(runs + 1):
                w0 = api.host_waits()
                t0 = time.perf_counter()
                last = call()
                if i:      # the first call is the warm-up
                    walls.append(time.perf_counter() - t0)
                    waits.append(api.host_waits() - w0)
            return statistics.median(walls) * 1e3, waits[-1], last
        legs = {"haplotypes": [], "composed": []}
        for _ in range(alternations):      # (the composition first: it is what a build without the new call times, in the same place of its process)
            ms, waits_b, (res, cons) = timed(composed)
            legs["composed"].append(ms)
            if have:
                ms, waits_a, hap = timed(lambda: api.polish_haplotypes(pl, sr))
                legs["haplotypes"].append(ms)
        pl.close()
    cig_words, bases, bb = int(res["cig_off"][-1]), int(res["base_off"][-1]), int(res["backbone_off"][-1])
    text = int(cons["cons_off"][-1])
    out = {"mode": "haplotypes", "config": cfg, "contigs": n, "runs": runs, "bundles": res["n_bundles"], "pieces": res["n_pieces"],
           "composed_wall_ms_medians": legs["composed"], "composed_host_waits_per_call": waits_b,
           # (what the two calls move: the pieces down and up again, the consensus route's tables up, the text and the bundles' figures down)
           "composed_bytes_down": bases + bb + 4 * cig_words + text + 32 * res["n_bundles"], "composed_bytes_up": bases + bb + 4 * cig_words + 56 * res["n_pieces"]}
    if have:
        st = hap["stats"]
        plan_bytes = 4 * cig_words + 40 * res["n_pieces"]      # CIGAR words in, 40 B a piece out
        out.update({"haplotypes_wall_ms_medians": legs["haplotypes"], "haplotypes_host_waits_per_call": waits_a, "rounds": st["n_rounds"], "sub_rounds": st["n_sub_rounds"],
                    "haplotypes_bytes_down": st["bytes_down"], "haplotypes_bytes_up": st["bytes_up"],
                    "k_cons_plan_and_layout": {"ms": st["plan_ms"], "algorithmic_bytes": plan_bytes},
                    "equal": bool(all((hap[k] == cons[k]).all() for k in ("cons_off", "cons", "trim_start", "trim_end", "n_sub", "n_del", "n_ins_bases", "n_low", "n_skipped")))})
        if st["plan_ms"] > 0:
            gbs = plan_bytes / (st["plan_ms"] * 1e-3) / 1e9
            out["k_cons_plan_and_layout"].update({"GBs": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBS})
    print(json.dumps(out))


def main_refine(argv):
    cfg = argv[0] if argv else "C4"
    n = int(argv[1]) if len(argv) > 1 else 60
    runs = max(5, int(argv[2])) if len(argv) > 2 else 5
    alternations = int(argv[3]) if len(argv) > 3 else 3
    from hairsplitter_amd import synth
    with tempfile.TemporaryDirectory() as td:
        contigs, files = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1), outdir=td)      # before the GPU is touched (forks)
        from hairsplitter_amd import api
        api.require_gpu()
        pl = api.PipelineGroups(contigs, 4)
        cv, sr = pl.run_fused(0.33, 0, rarest_strain_abundance=0.01)
        have = hasattr(api, "polish_refine")

        def timed(call):
            walls, waits, last = [], [], None
            for i in range(runs + 1):
                w0 = api.host_waits()
                t0 = time.perf_counter()
                last = call()
                if i:      # the first call is the warm-up
                    walls.append(time.perf_counter() - t0)
                    waits.append(api.host_waits() - w0)
            return statistics.median(walls) * 1e3, waits[-1], last
        legs = {p: [] for p in ((1, 2, 3) if have else (1,))}
        waits, last = {}, {}
        for _ in range(alternations):
            for p in legs:
                ms, waits[p], last[p] = timed((lambda: api.polish_haplotypes(pl, sr)) if p == 1 else (lambda p=p: api.polish_haplotypes(pl, sr, passes=p)))
                legs[p].append(ms)
        pl.close()
    one = last[1]
    out = {"mode": "refine", "config": cfg, "contigs": n, "runs": runs, "bundles": one["n_bundles"], "pieces": one["n_pieces"], "bases": int(one["base_off"][-1]),
           "passes": {}}
    for p in legs:
        st = last[p]["stats"]
        row = {"wall_ms_medians": legs[p], "host_waits_per_call": waits[p], "bytes_down": st["bytes_down"], "bytes_up": st["bytes_up"], "sub_rounds": st["n_sub_rounds"]}
        if p > 1:
            ps = last[p]["passes"]
            row["per_pass"] = {k: [float(x) for x in ps[k]] for k in ps if k != "n_passes"}
            gather_bytes = 2 * (2 * int(one["base_off"][-1])) + 16 * one["n_pieces"]      # queries and targets (about as long) read and written, the windows
            ms = float(ps["windows_ms"][1])
            row["k_refine_windows_and_gather"] = {"ms": ms, "algorithmic_bytes": gather_bytes}
            if ms > 0:
                gbs = gather_bytes / (ms * 1e-3) / 1e9
                row["k_refine_windows_and_gather"].update({"GBs": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBS})
            device = sum(float(ps[k][1]) for k in ("windows_ms", "align_ms", "cigar_ms", "plan_ms", "consensus_ms"))
            row["a1_share_of_pass_2"] = float(ps["align_ms"][1]) / device if device > 0 else None
            row["text_changed_by_the_last_pass"] = bool(len(last[p]["cons"]) != len(one["cons"]) or (last[p]["cons"] != one["cons"]).any())
        out["passes"][str(p)] = row
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "refine":
        return main_refine(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "consensus":
        return main_consensus(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "haplotypes":
        return main_haplotypes(sys.argv[2:])
    cfg = sys.argv[1] if len(sys.argv) > 1 else "C4"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    runs = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
    n = n or OWN.get(cfg, 50)
    import __graft_entry__ as ge
    from hairsplitter_amd import synth
    paths = ge.paths()
    with tempfile.TemporaryDirectory() as td:
        contigs, files = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1), outdir=td)      # before the GPU is touched (forks)
        from hairsplitter_amd import api
        api.require_gpu()
        pl = api.PipelineGroups(contigs, 4)
        cv, sr = pl.run_fused(0.33, 0, rarest_strain_abundance=0.01)
        samples = []
        for i in range(runs + 1):
            t0 = time.perf_counter()
            res = api.polish_inputs(pl, sr)
            wall = time.perf_counter() - t0
            if i:      # the first call is the warm-up
                samples.append((res["stats"], wall))
        st = res["stats"]
        piece_bytes = int(res["base_off"][-1]) + int(res["backbone_off"][-1])
        bytes_of = {"cut": 4 * st["cut_ops_read"] + 64 * st["n_tasks"], "gather": 2 * piece_bytes}      # ops read + task in / out; piece bytes in plus out
        out = {"config": cfg, "contigs": n, "aligned_bp": int(pl.aligned_bp), "runs": runs, "bundles": res["n_bundles"], "pieces": res["n_pieces"],
               "tasks": st["n_tasks"], "rounds": st["n_rounds"], "piece_bytes": piece_bytes, "cigar_words": int(res["cig_off"][-1]),
               "call_wall_ms_median": statistics.median(w for _, w in samples) * 1e3}
        for k in ("scan", "cut", "gather", "cigar"):
            ms = statistics.median(s[k + "_ms"] for s, _ in samples)
            out["k_polish_" + k] = {"ms_median": ms}
            if k in bytes_of and ms > 0:
                gbs = bytes_of[k] / (ms * 1e-3) / 1e9
                out["k_polish_" + k].update({"algorithmic_bytes": bytes_of[k], "GBs": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBS})
        pl.close()
        if os.path.exists(paths["ref_cnc"]):
            col, vcf, err, gro = (os.path.join(td, x) for x in ("v.col", "v.vcf", "err.txt", "reads_haplo.gro"))
            subprocess.run([paths["cv"], files["gfa"], files["reads"], files["sam"], "16", td, err, "0", "0", col, vcf, "0.33"], check=True, stdout=subprocess.DEVNULL)
            e = min(float(open(err).read().strip()), 0.15)
            subprocess.run([paths["sr"], col, "16", str(e), os.path.join(td, "no_ploidy"), "0", "0.01", "0", gro, "0"], check=True, stdout=subprocess.DEVNULL)
            out["reference_create_new_contigs"] = [reference_wall(paths, files, gro, td, t) for t in (1, 16)]
        print(json.dumps(out))


if __name__ == "__main__":
    main()
