"""Throughput of the A1 kernel at the shapes of the stage-5 call sites (create_new_contigs.cpp:558-629: the 300-base end of a
piece inside its polished version of a few kb; tools.cpp:515-534: 200 bases inside 300): pairs/s and DP cell updates/s of
hs_edlib_hw_align (HW + start location + path), next to the reference's edlib on one host core on a sample of the same pairs.
With a query length above 300 the pairs are READS against a contig window (the read with ~8 % substitutions, insertions and
deletions inside target_len bases): the banded sweeps and Hirschberg's cuts, one wavefront per read.
Usage: python tools/myers_bench.py [n_pairs=20000] [target_len=2000] [query_len=300]     (prints one JSON line)
       python tools/myers_bench.py nw [n_pairs=2048] [read_len=10000]: hs_edlib_align NW TASK_PATH of reads against a copy with
       ~6 % edits (edlib's default mode; these pairs go through Hirschberg's cuts), with k = -1 and with k = the largest distance
       of the batch (every pair within the bound: the same results, the first sweep's band sized from k).
       python tools/myers_bench.py bytes [n_pairs=2048] [read_len=10000] [n_symbols=5]: the pairs of the nw leg through
       hs_edlib_align (four codes), the same pairs as bytes with 1 % of the bases replaced by N through hs_edlib_align_bytes
       without equalities, and the same with N = A, C, G, T: pairs/s of each and the two ratios to the four-code run. With
       n_symbols above 5 the replaced bases become bytes outside ACGT drawn from n_symbols - 4 values (17 and more: the scratch
       table instead of the LDS table; the equalities then make the first of them equal to every base).
       python tools/myers_bench.py dist: hs_edit_distance (distance and first end location, offsets on the device) in NW and in HW
       on the 20 000 pairs of 300 x 2 000 of the first form (8 lanes per pair) and on the 2 048 reads of 10 kb of the nw leg (a
       wavefront per pair): pairs/s of each.
       python tools/myers_bench.py realign [contig_kb=200] [n_contigs=4] [depth=30]: one synthetic job (ONT reads as PAF lines) from its
       three files to a resident hs_cv_batch both ways: (a) hs_realign_paf, the SAM parser and hs_cv_batch_create
       (hs_cv_batch_create_sam), (b) hs_cv_batch_create_paf. Wall time of each (best of two), the phase times of (b), and the bytes
       each route brings from the device to the host."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def nw_pairs(n, rl):
    rng = np.random.default_rng(10)
    qs, ts = [], []
    for _ in range(n):
        q = rng.integers(0, 4, size=rl, dtype=np.uint8)
        u = rng.random(rl)
        t = q.copy()
        sub = u < 0.02
        t[sub] = (t[sub] + 1) & 3
        ins = np.flatnonzero((u >= 0.02) & (u < 0.04))
        keep = np.insert(~((u >= 0.04) & (u < 0.06)), ins, True)
        t = np.insert(t, ins, rng.integers(0, 4, size=len(ins), dtype=np.uint8))[keep]
        qs.append(q); ts.append(t)
    return qs, ts


def bytes_paths(n, rl, n_symbols):
    import torch
    from hairsplitter_amd import api
    api.require_gpu()
    lib = api.load()
    qs, ts = nw_pairs(n, rl)
    qo = np.zeros(n + 1, np.int64); to = np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in qs], out=qo[1:]); np.cumsum([len(x) for x in ts], out=to[1:])
    oo = qo + to
    codes_q, codes_t = np.concatenate(qs), np.concatenate(ts)
    rng = np.random.default_rng(11)
    others = np.array(([ord("N")] + [b for b in range(256) if b not in b"ACGTN"])[:max(1, n_symbols - 4)], dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def with_others(codes):      # identical lengths and edit positions: 1 % of the bases become bytes outside ACGT
        s = acgt[codes].copy()
        hit = rng.random(len(s)) < 0.01
        s[hit] = rng.choice(others, size=int(hit.sum()))
        return s
    bq, bt = with_others(codes_q), with_others(codes_t)
    eq = np.array([[ord("N"), b] for b in b"ACGT"], dtype=np.uint8)
    dev = "cuda:0"
    dd = torch.zeros(n, dtype=torch.int32, device=dev); ds, de, dn, dl = (torch.zeros_like(dd) for _ in range(4))
    dops = torch.zeros(int(oo[-1]), dtype=torch.uint8, device=dev)
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    out = {"mode": "NW", "task": "path", "pairs": n, "read_len": rl, "n_symbols": int(len(set(bq.tolist()) | set(bt.tolist())))}
    for label, q, t, e in (("four_codes", codes_q, codes_t, None), ("bytes", bq, bt, 0), ("bytes_N_equals_ACGT", bq, bt, len(eq))):
        dq = torch.from_numpy(q).to(dev); dt = torch.from_numpy(t).to(dev)
        tail = (api._p(dd), api._p(ds), api._p(de), api._p(dn), api._p(dops), hp(oo), api._p(dl), C.c_void_p(0))
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if e is None:
                api._check(lib.hs_edlib_align(api._p(dq), hp(qo), api._p(dt), hp(to), C.c_int32(n), C.c_int32(0), C.c_int32(2), C.c_int32(-1), *tail))
            else:
                api._check(lib.hs_edlib_align_bytes(api._p(dq), hp(qo), api._p(dt), hp(to), C.c_int32(n), C.c_int32(0), C.c_int32(2), C.c_int32(-1),
                                                    eq.ctypes.data_as(C.POINTER(C.c_uint8)) if e else None, C.c_int32(e), *tail))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        best = min(times[1:])
        out[label] = {"seconds": best, "pairs_per_s": n / best, "distance_mean": float(dd.float().mean().item())}
    for label in ("bytes", "bytes_N_equals_ACGT"):
        out[label]["ratio_to_four_codes"] = out[label]["pairs_per_s"] / out["four_codes"]["pairs_per_s"]
    print(json.dumps(out))


def nw_paths(n, rl):
    import torch
    from hairsplitter_amd import api
    api.require_gpu()
    lib = api.load()
    qs, ts = nw_pairs(n, rl)
    qo = np.zeros(n + 1, np.int64); to = np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in qs], out=qo[1:]); np.cumsum([len(x) for x in ts], out=to[1:])
    oo = qo + to
    dev = "cuda:0"
    dq = torch.from_numpy(np.concatenate(qs)).to(dev); dt = torch.from_numpy(np.concatenate(ts)).to(dev)
    dd = torch.zeros(n, dtype=torch.int32, device=dev); ds, de, dn, dl = (torch.zeros_like(dd) for _ in range(4))
    dops = torch.zeros(int(oo[-1]), dtype=torch.uint8, device=dev)
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    out = {"mode": "NW", "task": "path", "pairs": n, "read_len": rl, "target_len_mean": float(np.mean([len(x) for x in ts]))}
    ref = None
    for label, k in (("k_-1", -1), ("k_max_distance", None)):
        if k is None:
            k = int(dd.max().item())
            out["k"] = k
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api._check(lib.hs_edlib_align(api._p(dq), hp(qo), api._p(dt), hp(to), C.c_int32(n), C.c_int32(0), C.c_int32(2), C.c_int32(k),
                                          api._p(dd), api._p(ds), api._p(de), api._p(dn), api._p(dops), hp(oo), api._p(dl), C.c_void_p(0)))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        best = min(times[1:])
        res = (dd.cpu().numpy().copy(), dl.cpu().numpy().copy(), dops.cpu().numpy())
        if ref is None:
            ref = res
            out["distance_mean"] = float(res[0].mean())
        else:
            assert np.array_equal(ref[0], res[0]) and np.array_equal(ref[1], res[1]) and np.array_equal(ref[2], res[2])
        out[label] = {"seconds": best, "pairs_per_s": n / best}
    print(json.dumps(out))


def planted_pairs(n, tl, qn):
    """the query, with ~4 % substitutions, somewhere inside the target; above 300 bases 2 % deletions and 2 % insertions on top"""
    rng = np.random.default_rng(9)
    reads = qn > 300
    q = rng.integers(0, 4, size=(n, qn), dtype=np.uint8)
    t = rng.integers(0, 4, size=(n, tl), dtype=np.uint8)
    pos = rng.integers(0, tl - qn - (qn >> 4), size=n)
    for i in range(n):
        m = q[i].copy()
        e = rng.random(qn) < 0.04
        m[e] = (m[e] + 1) & 3
        if reads:
            keep = rng.random(qn) >= 0.02
            m = m[keep]
            ins = np.flatnonzero(rng.random(len(m)) < 0.02)
            m = np.insert(m, ins, rng.integers(0, 4, size=len(ins), dtype=np.uint8))
        t[i, pos[i]:pos[i] + len(m)] = m
    return q, t, pos


def distances():
    import torch
    from hairsplitter_amd import api
    api.require_gpu()
    lib = api.load()
    dev = "cuda:0"
    q, t, _ = planted_pairs(20000, 2000, 300)
    rq, rt = nw_pairs(2048, 10000)
    out = {"leg": "dist"}
    for label, qs, ts in (("pairs_300_in_2000", list(q), list(t)), ("reads_10kb", rq, rt)):
        n = len(qs)
        qo = np.zeros(n + 1, np.int64); to = np.zeros(n + 1, np.int64)
        np.cumsum([len(x) for x in qs], out=qo[1:]); np.cumsum([len(x) for x in ts], out=to[1:])
        dq, dqo, dt, dto = (torch.from_numpy(a).to(dev) for a in (np.concatenate(qs), qo, np.concatenate(ts), to))
        dd = torch.zeros(n, dtype=torch.int32, device=dev); de = torch.zeros_like(dd)
        out[label] = {"pairs": n}
        for mode, mi in (("NW", 0), ("HW", 2)):
            times = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                api._check(lib.hs_edit_distance(api._p(dq), api._p(dqo), api._p(dt), api._p(dto), C.c_int32(n), C.c_int32(mi), api._p(dd), api._p(de), C.c_void_p(0)))
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            best = min(times[1:])
            out[label][mode] = {"seconds": best, "pairs_per_s": n / best, "distance_mean": float(dd.float().mean().item()), "end_mean": float(de.float().mean().item())}
    print(json.dumps(out))


def realign(kb, nc, depth):
    import re
    import tempfile
    from hairsplitter_amd import api, synth
    api.require_gpu()
    lib = api.load()
    ops_re = re.compile(r"(\d+)([MIDNSHP=X])")

    class Stats(C.Structure):
        _fields_ = [("n_lines", C.c_int64), ("n_aligned", C.c_int64), ("query_bases", C.c_int64), ("ms_device", C.c_double), ("ms_total", C.c_double)]
    with tempfile.TemporaryDirectory() as td:
        cs = [synth.make_contig(51, i, kb * 1000, 2, 0.01, depth, "ont") for i in range(nc)]
        f = synth.write_files(cs, td)
        paf, sam = os.path.join(td, "a.paf"), os.path.join(td, "re.sam")
        d2h_a = 0      # route (a) brings the whole move buffer of every round back (query + window bytes per pair) and three ints per pair
        with open(paf, "w") as o:
            for c in cs:
                for a in c.alns:
                    qlen = len(c.reads[a.read])
                    op, ln = a.cigar & 0xF, (a.cigar >> 4).astype(np.int64)
                    refspan = int(ln[(op == 0) | (op == 2) | (op == 7) | (op == 8)].sum())
                    o.write("\t".join(map(str, [c.read_names[a.read], qlen, 0, qlen, "+" if a.strand else "-", c.name, 0, a.pos, a.pos + refspan, 0, refspan, 60])) + "\n")
                    d2h_a += qlen + (min(len(c.seq), a.pos + refspan + 100) - max(0, a.pos - 100)) + 12
        out = {"leg": "realign", "contigs": nc, "contig_kb": kb, "depth": depth, "records": sum(len(c.alns) for c in cs)}
        ta, tb, split_a, rec = [], [], None, None
        for _ in range(2):
            st = Stats()
            t0 = time.perf_counter()
            assert lib.hs_realign_paf(f["gfa"].encode(), f["reads"].encode(), paf.encode(), sam.encode(), C.c_int32(0), C.byref(st)) == 0, lib.hs_last_error()
            t1 = time.perf_counter()
            ba = api.CvBatch.from_sam(f["gfa"], f["reads"], sam)
            t2 = time.perf_counter()
            bp_a = ba.aligned_bp
            ba.close()
            if not ta or t2 - t0 < min(ta):
                split_a = {"realign_paf_s": t1 - t0, "of_which_device_s": st.ms_device / 1e3, "sam_parser_and_batch_create_s": t2 - t1, "sam_bytes": os.path.getsize(sam)}
            ta.append(t2 - t0)
            t0 = time.perf_counter()
            bb = api.CvBatch.from_paf(f["gfa"], f["reads"], paf)
            dt = time.perf_counter() - t0
            assert bb.aligned_bp == bp_a and bb.records["n_dropped"] == 0
            if not tb or dt < min(tb):
                rec = bb.records
            tb.append(dt)
            bb.close()
        n = rec["n_rec"]
        out["file_route"] = dict(split_a, wall_s=min(ta), d2h_bytes=d2h_a)
        out["resident_route"] = {"wall_s": min(tb), "d2h_bytes": 4 * rec["cigar_words"] + n * 12 + (n + rec["n_rounds"]) * 8,
                                 "cut_ms": rec["t_cut_ms"], "align_ms": rec["t_align_ms"], "cigar_ms": rec["t_cigar_ms"], "download_ms": rec["t_download_ms"],
                                 "rounds": rec["n_rounds"], "move_bytes_left_on_device": rec["move_bytes"], "cigar_words": rec["cigar_words"]}
        out["wall_ratio_file_over_resident"] = min(ta) / min(tb)
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "realign":
        return realign(*(int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 200), (3, 4), (4, 30))))
    if len(sys.argv) > 1 and sys.argv[1] == "nw":
        return nw_paths(int(sys.argv[2]) if len(sys.argv) > 2 else 2048, int(sys.argv[3]) if len(sys.argv) > 3 else 10000)
    if len(sys.argv) > 1 and sys.argv[1] == "bytes":
        return bytes_paths(int(sys.argv[2]) if len(sys.argv) > 2 else 2048, int(sys.argv[3]) if len(sys.argv) > 3 else 10000,
                           int(sys.argv[4]) if len(sys.argv) > 4 else 5)
    if len(sys.argv) > 1 and sys.argv[1] == "dist":
        return distances()
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    tl = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    import torch
    from hairsplitter_amd import api
    api.require_gpu()
    lib = api.load()
    qn = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    reads = qn > 300
    q, t, pos = planted_pairs(n, tl, qn)
    qo = np.arange(n + 1, dtype=np.int64) * qn
    to = np.arange(n + 1, dtype=np.int64) * tl
    oo = np.arange(n + 1, dtype=np.int64) * (qn + tl)
    dev = "cuda:0"
    dq = torch.from_numpy(q.reshape(-1)).to(dev); dt = torch.from_numpy(t.reshape(-1)).to(dev)
    dd = torch.zeros(n, dtype=torch.int32, device=dev); ds = torch.zeros_like(dd); de = torch.zeros_like(dd); dl = torch.zeros_like(dd)
    dops = torch.zeros(int(oo[-1]), dtype=torch.uint8, device=dev)
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    out = {"pairs": n, "query_len": qn, "target_len": tl}
    for path in (True, False):
        times = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api._check(lib.hs_edlib_hw_align(api._p(dq), hp(qo), api._p(dt), hp(to), C.c_int32(n), api._p(dd), api._p(ds), api._p(de),
                                             api._p(dops) if path else C.c_void_p(0), hp(oo), api._p(dl), C.c_void_p(0)))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        best = min(times[1:])
        # cells: sweep 1 over the whole target, sweep 2 over the prefix up to the end, sweep 3 over the aligned part
        end = de.cpu().numpy().astype(np.int64); st = ds.cpu().numpy().astype(np.int64)
        cells = float((tl + (end + 1) + ((end - st + 1) if path else 0)).sum()) * qn
        out["path" if path else "locations_only"] = {"seconds": best, "pairs_per_s": n / best, "GCUPS": cells / best / 1e9}
    assert int((np.abs(ds.cpu().numpy() - pos) <= (8 if reads else 0)).sum()) > 0.95 * n       # the planted placement is found
    ref = os.path.join(ROOT, "oracle", "_ref", "edlib_driver")
    if os.path.exists(ref):
        k = min(n, 300 if not reads else 40)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        lines = "".join("HWPATH -1 %s %s\n" % (acgt[q[i]].tobytes().decode(), acgt[t[i]].tobytes().decode()) for i in range(k))
        t0 = time.perf_counter()
        subprocess.run([ref], input=lines, capture_output=True, text=True, check=True)
        dt_ = time.perf_counter() - t0
        out["reference_edlib_one_core"] = {"pairs": k, "seconds": dt_, "pairs_per_s": k / dt_}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
