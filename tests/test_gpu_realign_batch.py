"""The CIGAR-less input in memory (hs_capi_realign.inc): intervals -> pairs cut on the device (k_realign_cut) -> A1 -> CIGAR words on the
device (hs_moves_to_cigar) -> records and a resident batch. (a) every record against the reference's own bundled edlib
(oracle/_ref/edlib_driver, HWPATH -1 <segment> <window>, the strings cut here in Python), the scheme of
tests/test_gpu_realign.py::test_realigned_records_equal_the_reference_edlib; (b) an interval the aligner has no path for; (c) the batch
of hs_cv_batch_create_paf against the batch made from the SAM hs_realign_paf writes for the same PAF; (d) refused input."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = 100
HS_EINVAL = -2
OPS = re.compile(r"(\d+)([MIDNSHP=X])")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
OPCODE = {"M": 0, "I": 1, "D": 2, "S": 4}


def _text(codes):
    return ACGT[np.asarray(codes, np.uint8)].tobytes().decode()


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _truth_intervals(contigs, clip):
    """(read, contig, strand, qs, qe, ts, te) of every truth alignment, reads numbered over all contigs; clip > 0 narrows both intervals"""
    out, base = [], 0
    for ci, c in enumerate(contigs):
        for a in c.alns:
            qlen = len(c.reads[a.read])
            ops, lens = a.cigar & 0xF, (a.cigar >> 4).astype(np.int64)
            refspan = int(lens[(ops == 0) | (ops == 2) | (ops == 7) | (ops == 8)].sum())
            qs, qe, ts, te = 0, qlen, a.pos, a.pos + refspan      # (these contigs carry no clips)
            if clip and qe - qs > 4 * clip and te - ts > 4 * clip:
                qs += clip; qe -= clip; ts += clip; te -= clip
            out.append((base + a.read, ci, 1 if a.strand else 0, qs, qe, ts, te))
        base += len(c.reads)
    return out


def _hand_made(contigs, rng):
    """short intervals on both strands: at the read's first base, at its last base, inside it; on the contig's first bases, its last
    bases (windows clamped there) and inside it"""
    out, base = [], [0]
    for c in contigs:
        base.append(base[-1] + len(c.reads))
    k = 0
    for n in (1, 2, 3, 5, 17, 63, 64, 65):
        for strand in (1, 0):
            for where in range(3):
                ci = k % len(contigs)
                c = contigs[ci]
                r = int(rng.integers(0, len(c.reads)))
                qlen, L = len(c.reads[r]), len(c.seq)
                qs = (0, qlen - n, int(rng.integers(1, qlen - n)))[(k + where) % 3]
                ts = (0, L - n, int(rng.integers(PAD + 1, L - n - PAD)))[where]
                out.append((base[ci] + r, ci, strand, qs, qs + n, ts, ts + n))
                k += 1
    return out


def _expected(contigs, intervals, driver):
    """per interval (pos, distance, words) from the reference's edlib on the strings cut in Python"""
    reads = [r for c in contigs for r in c.reads]
    lines, w0s = [], []
    for rd, ci, strand, qs, qe, ts, te in intervals:
        seg = _text(reads[rd][qs:qe])
        if not strand:
            seg = _revcomp(seg)
        L = len(contigs[ci].seq)
        w0, w1 = max(0, ts - PAD), min(L, te + PAD)
        lines.append("HWPATH -1 %s %s" % (seg, _text(contigs[ci].seq[w0:w1])))
        w0s.append(w0)
    ref = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(ref) == len(intervals)
    out = []
    for (rd, ci, strand, qs, qe, ts, te), w0, r in zip(intervals, w0s, ref):
        dist, start, end, ext = r.split()
        qlen = len(reads[rd])
        runs = []      # edlib's extended CIGAR (= X I D) folded to M / I / D runs
        for a, b in OPS.findall(ext):
            b = "M" if b in "=X" else b
            if runs and runs[-1][1] == b:
                runs[-1][0] += int(a)
            else:
                runs.append([int(a), b])
        cl, cr = (qs, qlen - qe) if strand else (qlen - qe, qs)
        runs = ([[cl, "S"]] if cl else []) + runs + ([[cr, "S"]] if cr else [])
        out.append((w0 + int(start), int(dist), np.array([(n << 4) | OPCODE[b] for n, b in runs], np.uint32)))
    return out


def _check_records(rec, intervals, want, skip=()):
    """records == the expectation of every interval not in `skip`, grouped by contig, input order inside a contig"""
    keep = [i for i in range(len(intervals)) if i not in skip]
    order = sorted(keep, key=lambda i: intervals[i][1])      # (sorted() is stable)
    assert rec["rec_interval"].tolist() == order
    n_contigs = rec["n_contigs"]
    counts = np.bincount([intervals[i][1] for i in keep], minlength=n_contigs)
    assert rec["contig_rec_off"].tolist() == np.concatenate(([0], np.cumsum(counts))).tolist()
    for k, i in enumerate(order):
        pos, dist, words = want[i]
        got = rec["cigar"][rec["rec_cig_off"][k]:rec["rec_cig_off"][k + 1]]
        assert rec["rec_read"][k] == intervals[i][0] and rec["rec_strand"][k] == intervals[i][2], (i, intervals[i])
        assert rec["rec_pos"][k] == pos and rec["rec_dist"][k] == dist, (i, intervals[i], rec["rec_pos"][k], pos, rec["rec_dist"][k], dist)
        assert np.array_equal(got, words), (i, intervals[i], got[:8], words[:8])
    assert rec["cigar_words"] == rec["rec_cig_off"][-1] == len(rec["cigar"])


@pytest.fixture(scope="module")
def job(built):
    from hairsplitter_amd import synth, api
    contigs = [synth.make_contig(41, 0, 14_000, 2, 0.01, 12, "ont"), synth.make_contig(41, 1, 9_000, 3, 0.01, 10, "ont")]
    rng = np.random.default_rng(41)
    intervals = _truth_intervals(contigs, 0) + _truth_intervals(contigs, 25) + _hand_made(contigs, rng)
    intervals = [intervals[i] for i in rng.permutation(len(intervals))]      # input order interleaves the two contigs
    driver = os.path.join(os.path.dirname(built["ref_cv"]), "edlib_driver")
    return {"contigs": contigs, "flat": api.FlatBatch(contigs), "intervals": intervals, "want": _expected(contigs, intervals, driver)}


def test_records_equal_the_reference_edlib(job):
    from hairsplitter_amd import api
    iv = job["intervals"]
    assert [c for _, c, *_ in iv] != sorted(c for _, c, *_ in iv)      # (the input interleaves the contigs)
    rec, batch = api.realign_intervals(job["flat"], iv, pad=PAD, want_batch=False)
    assert batch is None
    assert rec["n_dropped"] == 0 and rec["n_rec"] == rec["n_intervals"] == len(iv)
    _check_records(rec, iv, job["want"])
    assert rec["n_rounds"] == 1 and rec["move_bytes"] > 0


def test_an_interval_without_a_path_is_dropped(job):
    from hairsplitter_amd import api
    flat = job["flat"]
    rng = np.random.default_rng(5)
    long_read = rng.integers(0, 4, size=(1 << 20) + 1).astype(np.uint8)
    seqs = {"contig_seq": flat.contig_seq, "contig_off": flat.contig_off, "read_seq": np.concatenate((flat.read_seq, long_read)),
            "read_off": np.concatenate((flat.read_off, [flat.read_off[-1] + len(long_read)]))}
    at = len(job["intervals"]) // 2
    iv = job["intervals"][:at] + [(flat.n_reads, 1, 1, 0, len(long_read), 4000, 4100)] + job["intervals"][at:]
    want = job["want"][:at] + [None] + job["want"][at:]
    rec, batch = api.realign_intervals(seqs, iv, pad=PAD, want_batch=True)
    assert rec["n_dropped"] == 1 and rec["dropped"].tolist() == [at]
    assert rec["n_rec"] == len(iv) - 1
    _check_records(rec, iv, want, skip={at})
    assert batch is not None and batch.aligned_bp > 0      # the batch still builds
    batch.close()


def _sam_to_paf(sam, paf):
    """the PAF a mapper would print beside these SAM records (tests/test_gpu_realign.py)"""
    with open(sam) as f, open(paf, "w") as o:
        for l in f:
            if l.startswith("@"):
                continue
            t = l.rstrip("\n").split("\t")
            qlen = int([x for x in t if x.startswith("LN:i:")][0][5:])
            ops = [(int(a), b) for a, b in OPS.findall(t[5])]
            ls = ops[0][0] if ops[0][1] in "SH" else 0
            rs = ops[-1][0] if ops[-1][1] in "SH" else 0
            refspan = sum(a for a, b in ops if b in "MD=X")
            minus = int(t[1]) & 16
            qs, qe = (rs, qlen - ls) if minus else (ls, qlen - rs)
            ts = int(t[3]) - 1
            o.write("\t".join(map(str, [t[0], qlen, qs, qe, "-" if minus else "+", t[2], 0, ts, ts + refspan, 0, refspan, 60])) + "\n")


def test_batch_from_a_paf_equals_the_batch_from_the_sam_of_the_file_route(built):
    from hairsplitter_amd import synth, api
    lib = api.load()
    with tempfile.TemporaryDirectory() as td:
        c = [synth.make_contig(43, 0, 16_000, 2, 0.012, 30, "ont"), synth.make_contig(43, 1, 12_000, 3, 0.012, 32, "ont")]
        f = synth.write_files(c, td)
        paf, sam = os.path.join(td, "aln.paf"), os.path.join(td, "re.sam")
        _sam_to_paf(f["sam"], paf)
        assert lib.hs_realign_paf(f["gfa"].encode(), f["reads"].encode(), paf.encode(), sam.encode(), C.c_int32(4), None) == 0, lib.hs_last_error()
        # the FlatBatch of that SAM: its records replace the truth alignments of the contigs
        by_contig = {x.name: [] for x in c}
        for l in open(sam):
            if l.startswith("@"):
                continue
            t = l.rstrip("\n").split("\t")
            by_contig[t[2]].append(t)
        from_sam = []
        for x in c:
            idx = {nm: i for i, nm in enumerate(x.read_names)}
            alns = [synth.Alignment(idx[t[0]], int(t[3]) - 1, not (int(t[1]) & 16), np.array([(int(a) << 4) | "MIDNSHP=X".index(b) for a, b in OPS.findall(t[5])], np.uint32),
                                    int([v for v in t if v.startswith("NM:i:")][0][5:])) for t in by_contig[x.name]]
            assert len(alns) == len(x.alns)
            from_sam.append(dataclasses.replace(x, alns=alns))
        a = api.CvBatch.from_paf(f["gfa"], f["reads"], paf)
        b = api.CvBatch(api.FlatBatch(from_sam))
        assert a.records["n_dropped"] == 0 and a.aligned_bp == b.aligned_bp
        ra, rb = a.run(), b.run()
        a.close(); b.close()
        assert rb["snp_off"][-1] > 0
        for k in ("snp_off", "snp_pos", "snp_ref", "snp_alt", "col_off", "col_idx", "col_code", "mean_distance", "depth"):
            assert np.array_equal(ra[k], rb[k]), k
        assert ra["error_rate"] == rb["error_rate"]


def test_bad_input_is_refused(job):
    from hairsplitter_amd import api
    flat = job["flat"]
    good = job["intervals"][0]
    L1 = int(flat.contig_off[2] - flat.contig_off[1])
    bad = {"qstart >= qend": (good[0], good[1], good[2], 7, 7, good[5], good[6]),
           "tend > L": (good[0], 1, good[2], good[3], good[4], L1 - 50, L1 + 1),
           "read out of range": (flat.n_reads, good[1], good[2], good[3], good[4], good[5], good[6])}
    for what, iv in bad.items():
        with pytest.raises(api.HsError, match=r"error -2: hs_realign_intervals: interval 1 "):
            api.realign_intervals(flat, [good, iv], pad=PAD, want_batch=False)
    lib = api.load()
    one = np.zeros(1, np.int32); s = np.ones(1, np.uint8)
    out = C.c_void_p()
    p32, p8, p64 = (lambda a: api._hp(a, C.c_int32)), (lambda a: api._hp(a, C.c_uint8)), (lambda a: api._hp(a, C.c_int64))
    rc = lib.hs_realign_intervals(p8(flat.contig_seq), p64(flat.contig_off), C.c_int32(flat.n_contigs), p8(flat.read_seq), p64(flat.read_off), C.c_int32(flat.n_reads),
                                  p32(one), p32(one), p8(s), p32(one), p32(one), p32(one), p32(one), C.c_int32(-1), C.c_int32(PAD), C.byref(out), None)
    assert rc == HS_EINVAL


# ---- a job of more than one round: the same job in two rounds (a fresh process with the smallest chunk) and in one ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_ROUND_KEYS = ("contig_rec_off", "rec_interval", "rec_read", "rec_pos", "rec_dist", "rec_strand", "rec_cig_off", "cigar", "dropped", "n_pieces", "n_rounds")
N_TWO_ROUND = 9000
TWO_ROUND_CHILD = """
import sys
import numpy as np
from hairsplitter_amd import api
j = np.load(sys.argv[1])
seqs = {k: j[k] for k in ("contig_seq", "contig_off", "read_seq", "read_off")}
out = {}
for case, rec in (("plain", api.realign_intervals(seqs, j["intervals"], pad=int(j["pad"]), want_batch=False)[0]),
                  ("anchored", api.realign_intervals_anchored(seqs, j["intervals"], j["anc_off"], j["anc_q"], j["anc_t"], pad=int(j["pad"]), want_batch=False)[0])):
    for k in sys.argv[3:]:
        out[case + "_" + k] = np.asarray(rec[k])
np.savez(sys.argv[2], **out)
"""


def _two_round_job():
    """one contig of 3 000 bases; 50 reads of 1 000 bases cut from it with about 1 % substitutions (no indels), every second one reverse-complemented;
    9 000 intervals (read i % 50, whole read, its true span) whose windows (pad 100) all have their 1 200 bases; three anchors per interval on the true
    diagonal, at 250, 500 and 750 of the read as it aligns and of the span"""
    rng = np.random.default_rng(97)
    contig = rng.integers(0, 4, size=3000).astype(np.uint8)
    reads, rows = [], []
    for r in range(50):
        start = int(rng.integers(PAD, 3000 - 1000 - PAD + 1))
        seg = contig[start:start + 1000].copy()
        sub = rng.random(1000) < 0.01
        seg[sub] = (seg[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
        plus = r % 2 == 0
        reads.append(seg if plus else (3 - seg[::-1]).astype(np.uint8))
        rows.append((r, 0, 1 if plus else 0, 0, 1000, start, start + 1000))
    intervals = np.array([rows[i % 50] for i in range(N_TWO_ROUND)], np.int64)
    at = np.array([250, 500, 750], np.int64)
    return {"contig_seq": contig, "contig_off": np.array([0, 3000], np.int64), "read_seq": np.concatenate(reads), "read_off": np.arange(51, dtype=np.int64) * 1000,
            "intervals": intervals, "pad": np.int64(PAD), "anc_off": np.arange(N_TWO_ROUND + 1, dtype=np.int64) * 3, "anc_q": np.tile(at, N_TWO_ROUND).astype(np.int32),
            "anc_t": (intervals[:, 5:6] + at[None, :]).reshape(-1).astype(np.int32)}


@pytest.fixture(scope="module")
def two_rounds(built, tmp_path_factory):
    """the job's records from a child process whose rounds hold 16 MB of bases (the floor of HS_REALIGN_CHUNK_MB, read once per process), and the job"""
    job = _two_round_job()
    # the round bound of hs_capi_realign.inc on this job: an interval costs 1 000 + 1 200 bases and a round closes once it holds the chunk
    cost = (job["intervals"][:, 4] - job["intervals"][:, 3]) + (np.minimum(3000, job["intervals"][:, 6] + PAD) - np.maximum(0, job["intervals"][:, 5] - PAD))
    assert (cost == 2200).all()
    first = int(np.searchsorted(np.cumsum(cost) - cost, 16 << 20))
    assert (first, N_TWO_ROUND - first) == (7627, 1373)
    td = tmp_path_factory.mktemp("two_rounds")
    src, dst = str(td / "job.npz"), str(td / "records.npz")
    np.savez(src, **job)
    r = subprocess.run([sys.executable, "-c", TWO_ROUND_CHILD, src, dst, *TWO_ROUND_KEYS], cwd=ROOT, env=dict(os.environ, HS_REALIGN_CHUNK_MB="16"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return job, np.load(dst)


def _same_in_one_round(rec, child, case):
    assert int(child[case + "_n_rounds"]) == 2 and rec["n_rounds"] == 1
    assert rec["n_rec"] + rec["n_dropped"] == N_TWO_ROUND
    for k in TWO_ROUND_KEYS[:-1]:
        assert np.array_equal(np.asarray(rec[k]), child[case + "_" + k]), k


def test_two_rounds_equal_one_round(two_rounds):
    from hairsplitter_amd import api
    job, child = two_rounds
    rec, _ = api.realign_intervals(job, job["intervals"], pad=PAD, want_batch=False)
    _same_in_one_round(rec, child, "plain")
    assert rec["n_pieces"] == N_TWO_ROUND


def test_two_rounds_equal_one_round_anchored(two_rounds):
    from hairsplitter_amd import api
    job, child = two_rounds
    rec, _ = api.realign_intervals_anchored(job, job["intervals"], job["anc_off"], job["anc_q"], job["anc_t"], pad=PAD, want_batch=False)
    _same_in_one_round(rec, child, "anchored")
    assert rec["n_pieces"] == 4 * N_TWO_ROUND
