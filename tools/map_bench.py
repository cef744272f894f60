"""The read mapper (hs_map_reads, hs_map_to_batch; hs_kernels_map.hip) on a job of a bench configuration, held against the truth alignments of synth.py:
  1. the kernels' own times (HIP events around the minimizer, hit and vote launches), the algorithmic bytes each group moves and their share of 8 TB/s:
     minimizers 1 B per read base + 12 B per minimizer written; hits 8 B per minimizer read + 16 B per hit written and as much read back by the vote
     with 44 B per read written (the index's buckets, read at random, are not counted);
  2. reads per second of hs_map_reads and of hs_map_to_batch, and the share of the latter that A1 and the CIGAR words take;
  3. the host half of the same rule (tests/harness/map_selftest, 16 threads) on a sample of the reads, the only yardstick without another mapper;
  4. against the truth: the share of reads mapped, the share whose window [tstart - 100, tend + 100) holds the true span on the true contig and
     strand, the share of records whose (pos, CIGAR) equal those of hs_realign_intervals on the truth intervals;
  5. stages 3 and 4 on the mapped batch and on the truth-SAM batch: SNPs of each, SNP positions in common, the error rates; windows and groups of
     each, and the windows both have whose label arrays are equal element by element (a report, no assertion).
Usage: python tools/map_bench.py [config=C4] [contigs=16] [repeats=5] [host_sample=2000]      (prints one JSON line)
       python tools/map_bench.py [config=C4] [contigs=16] split [piece_len=20000]
The split mode cuts the contigs into pieces and keeps the reads and their truth: reads with more than one segment of hs_map_reads_split; aligned bp and
the mean depth over the last 1 000 bases of the pieces for the batch of hs_map_split_to_batch, of hs_map_to_batch and of the truth intervals; the vote
group's time (HIP events, medians of 5, alternating) split against plain on the cut job and on the uncut one, where nearly every read has one segment.
       python tools/map_bench.py [config=C4] [contigs=16] anchored [spacings=128,256,512,1024]
The anchored mode takes hs_map_to_batch and hs_map_to_batch_anchored in turn on the same reads, at spacing 128, 256, 512 and 1 024, five turns, one
process: wall from reads to batch, t_align_ms, the join's and k_map_anchors' time, the vote group's time, pieces, the sum of NM of both routes and the reads
above their optimum, stage 3 on both batches (medians, every run listed). The yardstick is the plain route of the same process."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def read_offset_at(cigar, pos, x):
    """read bases (contig orientation, clips included) in front of contig position x in an alignment that starts at pos"""
    q, t = 0, pos
    for w in cigar.tolist():
        op, n = w & 0xF, w >> 4
        in_ref, in_read = op in (0, 2, 3, 7, 8), op in (0, 1, 4, 7, 8)
        if in_ref and t + n > x:
            return q + (x - t if in_read else 0)
        t += n if in_ref else 0
        q += n if in_read else 0
    return q


def split_main(cfg, n, piece_len):
    """the contigs cut into pieces of piece_len, the reads as they were: what hs_map_reads_split adds at the pieces' ends"""
    import numpy as np
    from hairsplitter_amd import synth
    contigs, _ = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1))      # before the GPU is touched (forks)
    from hairsplitter_amd import api
    api.require_gpu()
    whole = api.FlatBatch(contigs)
    reads = (whole.read_seq, whole.read_off)
    R = whole.n_reads
    pieces, piece_of, truth, base = [], [], [], 0      # piece_of[c] = [(start, end, index)]
    for ci, c in enumerate(contigs):
        cuts = list(range(0, len(c.seq), piece_len))
        piece_of.append([(s, min(s + piece_len, len(c.seq)), len(pieces) + i) for i, s in enumerate(cuts)])
        pieces += [c.seq[s:s + piece_len] for s in cuts]
        for a in c.alns:
            ops, lens = a.cigar & 0xF, (a.cigar >> 4).astype(np.int64)
            end = a.pos + int(lens[(ops == 0) | (ops == 2) | (ops == 7) | (ops == 8)].sum())
            Lr = len(c.reads[a.read])
            for s, e, pi in piece_of[ci]:
                o0, o1 = max(a.pos, s), min(end, e)
                if o0 >= o1:
                    continue
                q0 = 0 if o0 == a.pos else read_offset_at(a.cigar, a.pos, o0)
                q1 = Lr if o1 == end else read_offset_at(a.cigar, a.pos, o1)
                if q1 > q0:
                    truth.append((base + a.read, pi, 1 if a.strand else 0) + ((q0, q1) if a.strand else (Lr - q1, Lr - q0)) + (o0 - s, o1 - s))
        base += len(c.reads)
    truth.sort(key=lambda x: (x[0], x[3]))
    tv = np.array(truth, np.int64)
    pseq, poff = api._flat(pieces)
    seqs = dict(contig_seq=pseq, contig_off=poff, read_seq=whole.read_seq, read_off=whole.read_off)
    plen = np.diff(poff)
    med = statistics.median

    def end_depth(rec):
        """mean depth over the last 1 000 bases of the pieces, from the records' positions and CIGAR words"""
        ops, lens = rec["cigar"] & 0xF, (rec["cigar"] >> 4).astype(np.int64)
        csum = np.concatenate(([0], np.cumsum(np.where((ops == 0) | (ops == 2) | (ops == 7) | (ops == 8), lens, 0))))
        span = csum[rec["rec_cig_off"][1:]] - csum[rec["rec_cig_off"][:-1]]
        L = plen[np.repeat(np.arange(len(plen)), np.diff(rec["contig_rec_off"]))]
        pos = rec["rec_pos"].astype(np.int64)
        lo = np.maximum(L - 1000, 0)
        cover = np.clip(np.minimum(pos + span, L) - np.maximum(pos, lo), 0, None)
        return float(cover.sum() / max(int((plen - np.maximum(plen - 1000, 0)).sum()), 1))

    out = {"config": cfg, "contigs": n, "piece_len": piece_len, "pieces": len(pieces), "reads": R, "truth_parts": len(tv)}
    with api.map_index((pseq, poff)) as ix:
        api.map_reads(ix, reads); api.map_reads_split(ix, reads)      # warm-up: pools, code object
        v_plain, v_split = [], []
        for _ in range(5):      # alternating, one process, one box
            v_plain.append(api.map_reads(ix, reads)["t_vote_ms"])
            seg = api.map_reads_split(ix, reads)
            v_split.append(seg["t_vote_ms"])
        b_split, rec_split, seg = api.map_split_to_batch(ix, reads)
        b_plain, rec_plain, res = api.map_to_batch(ix, reads)
    rec_truth, b_truth = api.realign_intervals(seqs, tv)
    n_seg = np.diff(seg["seg_off"])
    out["cut"] = {"reads_with_more_than_one_segment": int((n_seg > 1).sum()), "reads_without_a_segment": int((n_seg == 0).sum()), "segments": int(n_seg.sum()),
                  "reads_through_scratch_route": seg["n_wide"], "hits": seg["total_hits"],
                  "aligned_bp": {"split": b_split.aligned_bp, "plain": b_plain.aligned_bp, "truth": b_truth.aligned_bp},
                  "mean_depth_last_1000": {"split": round(end_depth(rec_split), 3), "plain": round(end_depth(rec_plain), 3), "truth": round(end_depth(rec_truth), 3)},
                  "dropped": {"split": int(rec_split["n_dropped"]), "plain": int(rec_plain["n_dropped"]), "truth": int(rec_truth["n_dropped"])},
                  "vote_ms": {"plain": round(med(v_plain), 4), "split": round(med(v_split), 4), "ratio": round(med(v_split) / med(v_plain), 3), "plain_all": [round(x, 4) for x in v_plain],
                              "split_all": [round(x, 4) for x in v_split]}}
    for b in (b_split, b_plain, b_truth):
        b.close()
    # the yardstick: the uncut job, where nearly every read has one segment
    with api.map_index((whole.contig_seq, whole.contig_off)) as ix:
        api.map_reads(ix, reads); api.map_reads_split(ix, reads)
        v_plain, v_split = [], []
        for _ in range(5):
            v_plain.append(api.map_reads(ix, reads)["t_vote_ms"])
            seg = api.map_reads_split(ix, reads)
            v_split.append(seg["t_vote_ms"])
    n_seg = np.diff(seg["seg_off"])
    out["uncut"] = {"reads_with_more_than_one_segment": int((n_seg > 1).sum()), "hits": seg["total_hits"],
                    "vote_ms": {"plain": round(med(v_plain), 4), "split": round(med(v_split), 4), "ratio": round(med(v_split) / med(v_plain), 3),
                                "plain_all": [round(x, 4) for x in v_plain], "split_all": [round(x, 4) for x in v_split]}}
    print(json.dumps(out))


def anchored_main(cfg, n, spacings=(128, 256, 512, 1024), turns=5):
    """hs_map_to_batch against hs_map_to_batch_anchored at every spacing, alternating inside one process"""
    import numpy as np
    from hairsplitter_amd import synth
    contigs, _ = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1))      # before the GPU is touched (forks)
    from hairsplitter_amd import api
    api.require_gpu()
    flat = api.FlatBatch(contigs)
    reads = (flat.read_seq, flat.read_off)
    med = statistics.median
    routes = ["plain"] + ["s%d" % s for s in spacings]
    runs = {k: {"wall_ms": [], "align_ms": [], "cut_ms": [], "cigar_ms": [], "join_ms": [], "anchors_ms": [], "vote_ms": []} for k in routes}
    last = {}

    def one(ix, key):
        t0 = time.perf_counter()
        if key == "plain":
            batch, rec, res = api.map_to_batch(ix, reads)
            anc = None
        else:
            batch, rec, res, anc = api.map_to_batch_anchored(ix, reads, api.map_anchor_params(spacing=int(key[1:])))
        dt = (time.perf_counter() - t0) * 1e3
        r = runs[key]
        r["wall_ms"].append(dt); r["align_ms"].append(rec["t_align_ms"]); r["cut_ms"].append(rec["t_cut_ms"]); r["cigar_ms"].append(rec["t_cigar_ms"])
        r["join_ms"].append(rec["t_join_ms"]); r["anchors_ms"].append(anc["t_anchors_ms"] if anc else 0.0); r["vote_ms"].append(res["t_vote_ms"])
        if key in last:
            last[key][0].close()
        last[key] = (batch, rec, res, anc)

    with api.map_index((flat.contig_seq, flat.contig_off)) as ix:
        for key in routes:      # warm-up: pools, code object
            one(ix, key)
        for r in runs.values():
            for v in r.values():
                v.clear()
        for _ in range(turns):
            for key in routes:
                one(ix, key)

    def nm_by_read(rec):
        return dict(zip(rec["rec_read"].tolist(), rec["rec_dist"].tolist()))

    def snps(r):
        return set((int(c), int(p)) for c in range(len(r["snp_off"]) - 1) for p in r["snp_pos"][r["snp_off"][c]:r["snp_off"][c + 1]])
    plain_nm = nm_by_read(last["plain"][1])
    plain_run = last["plain"][0].run()
    plain_snps = snps(plain_run)
    out = {"config": cfg, "contigs": n, "reads": flat.n_reads, "read_bases": int(flat.read_off[-1]), "turns": turns, "routes": {}}
    for key in routes:
        batch, rec, res, anc = last[key]
        nm = nm_by_read(rec)
        run = plain_run if key == "plain" else batch.run()
        sn = snps(run)
        out["routes"][key] = {
            **{k: round(med(v), 3) for k, v in runs[key].items()}, "wall_ms_all": [round(x, 1) for x in runs[key]["wall_ms"]], "align_ms_all": [round(x, 1) for x in runs[key]["align_ms"]],
            "records": int(rec["n_rec"]), "dropped": int(rec["n_dropped"]), "pieces": int(rec["n_pieces"]), "rounds": int(rec["n_rounds"]),
            "anchors": int(anc["anc_off"][-1]) if anc else 0, "reads_without_anchors": int((np.diff(anc["anc_off"])[res["contig"] >= 0] == 0).sum()) if anc else None,
            "sum_nm": int(sum(nm.values())), "reads_above_plain_nm": int(sum(1 for r, v in nm.items() if v > plain_nm.get(r, v))),
            "reads_below_plain_nm": int(sum(1 for r, v in nm.items() if v < plain_nm.get(r, v))),
            "snps": len(sn), "snps_in_common_with_plain": len(sn & plain_snps), "error_rate": float(run["error_rate"])}
        batch.close()
    # the reads that have anchors alone, records only (no batch): a mapped read without anchors goes the plain way on either route, and the few reads
    # that match their window nowhere cost a plain call most of its time
    res, anc = last[routes[1]][2], last[routes[1]][3]
    iv_all = api.map_intervals(res)
    has = np.diff(anc["anc_off"])[iv_all[:, 0]] > 0
    iv = iv_all[has]
    sub = {k: {"wall_ms": [], "align_ms": [], "join_ms": []} for k in routes}
    picks = {}
    for key in routes[1:]:
        a = last[key][3]
        n_anc = np.diff(a["anc_off"])[iv[:, 0]]
        idx = np.concatenate([np.arange(a["anc_off"][r], a["anc_off"][r + 1]) for r in iv[:, 0]]) if len(iv) else np.zeros(0, np.int64)
        picks[key] = (np.concatenate([[0], np.cumsum(n_anc)]).astype(np.int64), a["anc_q"][idx], a["anc_t"][idx])

    def one_sub(key):
        t0 = time.perf_counter()
        rec, _ = api.realign_intervals(flat, iv, want_batch=False) if key == "plain" else api.realign_intervals_anchored(flat, iv, *picks[key], want_batch=False)
        sub[key]["wall_ms"].append((time.perf_counter() - t0) * 1e3); sub[key]["align_ms"].append(rec["t_align_ms"]); sub[key]["join_ms"].append(rec["t_join_ms"])
        return rec
    for key in routes:
        one_sub(key)
    for r in sub.values():
        for v in r.values():
            v.clear()
    nm_sub = {}
    for _ in range(turns):
        for key in routes:
            nm_sub[key] = int(one_sub(key)["rec_dist"].sum())
    out["reads_with_anchors_only"] = {"intervals": int(len(iv)), "left_out": int((~has).sum()), "routes": {
        key: {**{k: round(med(v), 3) for k, v in sub[key].items()}, "wall_ms_all": [round(x, 1) for x in sub[key]["wall_ms"]], "align_ms_all": [round(x, 1) for x in sub[key]["align_ms"]],
              "sum_nm": nm_sub[key]} for key in routes}}
    print(json.dumps(out))


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "C4"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    if len(sys.argv) > 3 and sys.argv[3] == "anchored":
        return anchored_main(cfg, n, *([tuple(int(x) for x in sys.argv[4].split(","))] if len(sys.argv) > 4 else []))
    if len(sys.argv) > 3 and sys.argv[3] == "split":
        return split_main(cfg, n, int(sys.argv[4]) if len(sys.argv) > 4 else 20000)
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    sample = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    import numpy as np
    from hairsplitter_amd import synth
    contigs, _ = synth.generate_job(cfg, list(range(n)), workers=min(16, os.cpu_count() or 1))      # before the GPU is touched (forks)
    import map_cases as mc
    from hairsplitter_amd import api
    import __graft_entry__ as ge
    api.require_gpu()
    flat = api.FlatBatch(contigs)
    R, bases = flat.n_reads, int(flat.read_off[-1])
    reads = (flat.read_seq, flat.read_off)
    med = statistics.median
    t0 = time.perf_counter()
    ix = api.map_index((flat.contig_seq, flat.contig_off))
    t_index = (time.perf_counter() - t0) * 1e3
    api.map_reads(ix, reads)      # warm-up: pools, code object
    t_map, k_mz, k_hits, k_vote = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = api.map_reads(ix, reads)
        t_map.append(time.perf_counter() - t0)
        k_mz.append(res["t_minimizers_ms"]); k_hits.append(res["t_hits_ms"]); k_vote.append(res["t_vote_ms"])
    t_batch, a1_share = [], []
    for _ in range(max(1, reps // 2)):
        t0 = time.perf_counter()
        batch, rec, res_b = api.map_to_batch(ix, reads)
        dt = time.perf_counter() - t0
        t_batch.append(dt)
        a1_share.append((rec["t_align_ms"] + rec["t_cigar_ms"] + rec["t_cut_ms"]) / (dt * 1e3))
        if _ < max(1, reps // 2) - 1:
            batch.close()
    M, H = res["total_minimizers"], res["total_hits"]

    def group(ms, nbytes):
        return {"ms": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e6), 1) if ms > 0 else None,
                "share_of_8_TB_per_s": round(nbytes / (ms * 1e6) / 8000, 4) if ms > 0 else None}
    kernels = {"minimizers": group(med(k_mz), bases + 12 * M), "hits": group(med(k_hits), 8 * M + 16 * H), "vote": group(med(k_vote), 16 * H + 44 * R)}
    # ---- the truth ----
    truth_iv, base = [], 0
    for ci, c in enumerate(contigs):
        for a in c.alns:
            ops, lens = a.cigar & 0xF, (a.cigar >> 4).astype(np.int64)
            span = int(lens[(ops == 0) | (ops == 2) | (ops == 7) | (ops == 8)].sum())
            truth_iv.append((base + a.read, ci, 1 if a.strand else 0, 0, len(c.reads[a.read]), a.pos, a.pos + span))
        base += len(c.reads)
    tv = np.array(truth_iv, np.int64)
    order = np.argsort(tv[:, 0], kind="stable")
    tv = tv[order]
    assert np.array_equal(tv[:, 0], np.arange(R))      # one truth alignment per read
    mapped = res["contig"] >= 0
    holds = mapped & (res["contig"] == tv[:, 1]) & (res["strand"] == tv[:, 2]) & (res["tstart"] - 100 <= tv[:, 5]) & (tv[:, 6] <= res["tend"] + 100)
    rec_t, _ = api.realign_intervals(flat, tv, want_batch=False)

    def by_read(r):
        return {int(rd): (int(r["rec_pos"][k]), r["cigar"][r["rec_cig_off"][k]:r["rec_cig_off"][k + 1]].tobytes()) for k, rd in enumerate(r["rec_read"])}
    a, b = by_read(rec), by_read(rec_t)
    same_rec = sum(1 for rd, v in a.items() if b.get(rd) == v)
    # ---- the host half of the rule on a sample ----
    pick = np.linspace(0, R - 1, min(sample, R)).astype(np.int64)
    sub = [flat.read_seq[flat.read_off[i]:flat.read_off[i + 1]] for i in pick]
    cs = [flat.contig_seq[flat.contig_off[c]:flat.contig_off[c + 1]] for c in range(flat.n_contigs)]
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        mc.write_job(f.name, mc.params(), cs, sub, threads=16)
        import subprocess
        t0 = time.perf_counter()
        out = subprocess.run([ge.paths()["map_selftest"], f.name], stdout=subprocess.PIPE, check=True).stdout.decode()
        t_host = time.perf_counter() - t0
    host_rows = {int(t[1]): [int(x) for x in t[2:8]] for t in (l.split() for l in out.splitlines()) if t[0] == "R"}
    host_same = all(host_rows[k] == [int(res[f][i]) for f in ("contig", "strand", "qstart", "qend", "tstart", "tend")] for k, i in enumerate(pick))
    # ---- stages 3 and 4 on both batches ----
    truth_batch = api.CvBatch(flat)
    ra, rb = batch.run(), truth_batch.run()
    (_, s4a), (_, s4b) = batch.run_pipeline(), truth_batch.run_pipeline()
    batch.close(); truth_batch.close(); ix.close()

    def windows(sr):
        out = {}
        for c in range(len(sr["win_off"]) - 1):
            for w in range(int(sr["win_off"][c]), int(sr["win_off"][c + 1])):
                out[(c, int(sr["win_start"][w]), int(sr["win_end"][w]))] = sr["labels"][int(sr["label_off"][w]):int(sr["label_off"][w + 1])]
        return out
    wa, wb = windows(s4a), windows(s4b)
    n_groups = lambda ws: int(sum(len(set(v[v >= 0].tolist())) for v in ws.values()))
    both = [k for k in wa if k in wb]

    def snps(r):
        return set((int(c), int(p)) for c in range(len(r["snp_off"]) - 1) for p in r["snp_pos"][r["snp_off"][c]:r["snp_off"][c + 1]])
    sa, sb = snps(ra), snps(rb)
    print(json.dumps({
        "config": cfg, "contigs": n, "reads": R, "read_bases": bases, "contig_bases": int(flat.contig_off[-1]), "index_create_ms": round(t_index, 2),
        "minimizers": M, "hits": H, "reads_through_scratch_route": res["n_wide"], "kernels": kernels,
        "map_reads": {"ms": round(med(t_map) * 1e3, 2), "reads_per_s": round(R / med(t_map)), "Mbases_per_s": round(bases / med(t_map) / 1e6, 1)},
        "map_to_batch": {"ms": round(med(t_batch) * 1e3, 2), "reads_per_s": round(R / med(t_batch)), "share_of_A1_cut_and_cigar": round(med(a1_share), 3)},
        "host_rule_16_threads": {"reads": len(pick), "s_with_index_and_text_io": round(t_host, 3), "equals_device": bool(host_same)},
        "truth": {"share_mapped": round(float(mapped.mean()), 5), "share_window_holds_true_span": round(float(holds.mean()), 5),
                  "share_records_equal_truth_interval_records": round(same_rec / max(len(b), 1), 5), "records": len(a), "dropped": int(rec["n_dropped"])},
        "stage3": {"snps_mapped_batch": len(sa), "snps_truth_batch": len(sb), "snps_in_common": len(sa & sb),
                   "error_rate_mapped": float(ra["error_rate"]), "error_rate_truth": float(rb["error_rate"])},
        "stage4": {"windows_mapped_batch": len(wa), "windows_truth_batch": len(wb), "windows_in_common": len(both), "groups_mapped_batch": n_groups(wa),
                   "groups_truth_batch": n_groups(wb), "common_windows_with_equal_label_arrays": int(sum(np.array_equal(wa[k], wb[k]) for k in both))}}))


if __name__ == "__main__":
    main()
