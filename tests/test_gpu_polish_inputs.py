"""hs_polish_inputs (k_polish_cut / k_polish_gather / k_polish_cigar) on the device:
 1. against the bytes the reference's own HS_create_new_contigs handed to its polisher (tests/golden/polish_inputs, recorded by
    tools/record_polish_goldens.py): the multiset of the bundles that have at least one read;
 2. against the per-base restatement of create_new_contigs.cpp:358-521 (polish_restatement.py), the only oracle of the clipped
    CIGAR, startPosition, the cut points and the dropped list, on synthetic records that sit on every edge of the walk;
 3. plumbing: the tool's file, a call split by HS_POLISH_CHUNK_MB, contig sub-ranges.

One rule of the issue's list reads differently in the reference: a deletion that covers the whole range does not drop the read. The
walk takes the start and the end inside the deletion at the same read position, and :444 drops a read only when the start is
beyond the end or was never taken, so such a read stays with an empty piece (left out of reads_<id>.fasta, tools.cpp:357). The
reads that ARE dropped are those whose walk never reaches leftToPolish; the group whose reads are all dropped is made of them."""
import functools
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import polish_goldens as pg
import polish_restatement as pr

pytestmark = pytest.mark.gpu

OPS = {c: i for i, c in enumerate(pr.OPCHAR)}


# ---- 1. the reference's own bytes -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tool_bundles(run):
    from hairsplitter_amd import api
    source, polish = next((s, p) for r, s, p in pg.run_names() if r == run)
    with tempfile.TemporaryDirectory() as td:
        gfa, reads, sam, gro = pg.prepare(source, td)
        out = os.path.join(td, "polish.txt")
        api.polish_inputs_from_files(gfa, reads, sam, gro, out, polish_everything=bool(polish))
        restated = pr.job_bundles(gfa, reads, sam, gro, bool(polish)) if run in FULLY_COMPARED else None
        return pr.parse_tool_output(out), restated


@pytest.mark.parametrize("run", [r[0] for r in pg.recorded_runs()])
def test_bundles_are_the_reference_bytes(built, run):
    rec = pg.load(run)
    mine = sorted(pr.bundle_key(b["to_polish"].encode(), [(k, s.encode()) for k, _, _, s in b["pieces"]])
                  for b in _tool_bundles(run)[0] if int(b["head"][-1]) > 0)
    assert mine == rec["keys"]


def test_linked_with_polish_everything_is_recorded():
    assert "linked_p1" in [r[0] for r in pg.recorded_runs()]


FULLY_COMPARED = ("linked_p1", "clips_p0", "edge_ops_p1", "multi_p1", "dip10k_fastq_p1", "linked_rough_2_1_p1")


def _text_of_restated(b, name):
    """a restated bundle as the tool writes it"""
    head = [name] + [str(b[k]) for k in ("start", "end", "group", "left", "right", "overhang_left", "overhang_right")] + [str(len(b["pieces"]))]
    return {"head": head, "to_polish": b["to_polish"],
            "pieces": [(k, p["sam_pos"], p["cigar"], p["bases"]) for k, p in enumerate(b["pieces"]) if p["bases"]]}


@pytest.mark.parametrize("run", FULLY_COMPARED)
def test_golden_jobs_against_the_restatement(built, run):
    """every bundle of the job, the empty ones too, with startPosition and the clipped CIGAR of every read"""
    mine, (bundles, _, names) = _tool_bundles(run)
    assert mine == [_text_of_restated(b, names[b["contig"]]) for b in bundles]


# ---- 2. synthetic records ----------------------------------------------------------------------------
def _rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _read_len(cigar):
    n, num = 0, ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            if ch in "MISH=X":      # H as well: the batch refuses a CIGAR that runs past its read, and counts H as the pileup walks it
                n += int(num)
            num = ""
    return n


def _cigar_words(cigar):
    out, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num) << 4) | OPS[ch])
            num = ""
    return np.asarray(out, np.uint32)


LONG = "2M1I2M1D" * 50      # 200 ops, 4 ops move the reference cursor by 5: op 64 begins 80 bases, op 128 160 bases after the start
PIECE_LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097)


def _piece_cigar(n):
    return "4D3S" if n == 0 else "1M3S" if n == 1 else "1M%dI3S" % (n - 1)


# (pos, cigar, early): records of the 600-base contig; windows A (0,199) B (200,399) C (400,549) D (550,600) give
# leftToPolish 0 / 50 / 250 and rightToPolish 350 / 550 / 599. early: the walk of window C never reaches 250
CTG600 = (
    [(300, "200M", 0), (0, "120M", 1), (40, "7S300M", 0), (40, "5H300M", 0), (100, "300M9S", 0),
     (20, "30M3I400M", 0),      # an insertion exactly at leftToPolish of B: inside the piece
     (500, "50M4I30M", 0),      # an insertion exactly at rightToPolish of B: the piece ends before it
     (220, "30M5I100M", 0),     # the same at leftToPolish of C
     (30, "10M30D300M", 0),     # a deletion across leftToPolish of B
     (400, "140M20D30M", 0),    # a deletion across rightToPolish of B
     (10, "20M560D10M", 0),     # a deletion over the whole range of B (and over both bounds of C): an empty piece
     (0, "30M", 1), (0, "10M5S", 1),      # end before leftToPolish of B and C: dropped there
     (60, "50=3X40=10N100=", 0), (10, "100M20=5X10N100M2P30M", 0), (340, "10M5N10M", 0),
     (0, "30M0I20M0D300M", 0), (60, "10M10M5I5I3D2D100M", 0),      # ops without chars, neighbouring ops of one code
     (0, "600M", 0), (0, "3S600M2S", 0), (599, "1M", 0), (350, "5M", 0), (349, "5M", 0), (550, "4M", 0)] +
    [(p, LONG, 0) for p in (20, 80, 169, 170, 171, 190, 270, 300, 349)] +      # cut points in chunk 0, at op 63 / 64, in chunk 2
    [(90, "%dS300M%dS" % (k, (16 - (300 + k) % 16) % 16), 0) for k in range(16)] +      # every residue of the source offset mod 16 (read lengths are multiples of 16)
    [(100, _piece_cigar(n), 1) for n in PIECE_LENGTHS] +
    [(260, "1M%dI100M" % (n - 101), 0) for n in (4095, 4096, 4097)])
CTG100 = [(0, "100M", 0), (10, "5S60M2I20M", 0), (95, "5M", 0), (0, "3H50M10D30M", 0), (0, "99M1S", 0), (99, "1M", 0), (20, "30M", 0),
          (0, "40M", 0), (49, "2M3I2M", 0), (0, "20M70D10M", 0)]
CTG300 = [(0, "300M", 0), (100, "4S50M3D50M", 0), (299, "1M", 0), (0, "150M150I150M", 0)]


class Job:
    """contigs, reads, records and windows; as text (files) and as the arrays of the C ABI"""

    def __init__(self, seed=7, big=False):
        rng = random.Random(seed)
        self.contigs = []      # (name, raw sequence, records [(read index, strand, pos, cigar)], windows [(start, end, labels)] or None)
        self.reads = []        # (name, raw sequence)

        def records_of(specs, noisy):
            recs, early = [], []
            for pos, cigar, e in specs:
                for strand in (True, False):
                    self.reads.append(("r%d" % len(self.reads), _rand_seq(rng, _read_len(cigar), "ACGTacgtNnRY" if noisy else "ACGT")))
                    recs.append((len(self.reads) - 1, strand, pos, cigar))
                    early.append(e)
            return recs, early
        if big:      # three contigs of 0.5 MB of pieces each
            for c in range(3):
                recs, _ = records_of([(100, "1M60000I3S", 0)] * 4, False)
                self.contigs.append(("big%d" % c, _rand_seq(rng, 600), recs, [(0, 299, [r % 2 for r in range(len(recs))]), (300, 600, [0] * len(recs))]))
            return
        recs, early = records_of(CTG600, True)
        recs.append((recs[0][0], True, 5, "150M"))      # a second record of the first read: it carries the read's labels (the last one does)
        early.append(0)
        n = len(recs)
        lab_a = [-2 if r % 7 == 3 else -1 if r % 11 == 5 else r % 2 for r in range(n)]
        lab_b = [r % 3 for r in range(n)]
        lab_c = [2 if early[r] else r % 2 for r in range(n)]      # group 2 of window C: all of its reads are dropped
        lab_d = [-1 if r % 2 else -2 for r in range(n)]           # no label above -1
        self.contigs.append(("ctg600", _rand_seq(rng, 600, "ACGTacgtN"), recs, [(0, 199, lab_a), (200, 399, lab_b), (400, 549, lab_c), (550, 600, lab_d)]))
        recs, _ = records_of(CTG100, False)
        self.contigs.append(("ctg100", _rand_seq(rng, 100), recs, [(0, 49, [r % 2 for r in range(len(recs))]), (50, 100, [r % 3 for r in range(len(recs))])]))
        recs, _ = records_of(CTG300, False)
        self.contigs.append(("ctg300_nopartitions", _rand_seq(rng, 300), recs, None))      # polish_everything: the default interval (0, L)
        recs, _ = records_of([(0, "50M", 0)], False)
        self.contigs.append(("ctg_nowindows", _rand_seq(rng, 80), recs, []))                # in the .gro, without a GROUP line
        self.contigs.append(("ctg_norecords", _rand_seq(rng, 80), [], None))

    def write(self, td):
        p = {k: os.path.join(td, k) for k in ("assembly.gfa", "reads.fasta", "aln.sam", "x.gro")}
        with open(p["assembly.gfa"], "w") as f:
            for name, seq, _, _ in self.contigs:
                f.write("S\t%s\t%s\n" % (name, seq))
        with open(p["reads.fasta"], "w") as f:
            for name, seq in self.reads:
                f.write(">%s\n%s\n" % (name, seq))
        with open(p["aln.sam"], "w") as f:
            for name, seq, recs, _ in self.contigs:
                for rd, strand, pos, cigar in recs:
                    f.write("%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\tNM:i:0\tLN:i:%d\n" % (self.reads[rd][0], 0 if strand else 16, name, pos + 1, cigar,
                                                                                       max(100, len(self.reads[rd][1]))))
        with open(p["x.gro"], "w") as f:
            for name, seq, recs, wins in self.contigs:
                if wins is None:
                    continue
                f.write("CONTIG\t%s\t%d\t10\n" % (name, len(seq)))
                for rd, strand, pos, cigar in recs:
                    f.write("READ\t%s\t0\t0\t0\t0\t%d\n" % (self.reads[rd][0], 1 if strand else 0))
                for start, end, lab in wins:
                    idx = [r for r in range(len(lab)) if lab[r] != -2]
                    f.write("GROUP\t%d\t%d\t%s\t%s\n" % (start, end, "".join("%d," % r for r in idx) or ",", "".join("%d," % lab[r] for r in idx) or ","))
        return p["assembly.gfa"], p["reads.fasta"], p["aln.sam"], p["x.gro"]

    def flat(self):
        from hairsplitter_amd import api, synth
        code = {c: i for i, c in enumerate("ACGT")}

        def codes(raw):
            return np.asarray([code[c] for c in pr.sequence_str(raw)], np.uint8)
        out = []
        for name, seq, recs, _ in self.contigs:
            local = sorted(set(r[0] for r in recs))
            out.append(synth.ContigData(name, codes(seq), [codes(self.reads[r][1]) for r in local], [self.reads[r][0] for r in local],
                                        [synth.Alignment(local.index(rd), pos, strand, _cigar_words(cigar), 0) for rd, strand, pos, cigar in recs],
                                        np.zeros(len(local), np.int32)))
        return api.FlatBatch(out)

    def sr(self):
        win_off, ws, we, label_off, labels, has = [0], [], [], [0], [], []
        for name, seq, recs, wins in self.contigs:
            has.append(0 if wins is None else 1)
            for start, end, lab in (wins or []):
                ws.append(start); we.append(end); labels += lab; label_off.append(len(labels))
            win_off.append(len(ws))
        return ({"win_off": np.asarray(win_off, np.int64), "win_start": np.asarray(ws, np.int32), "win_end": np.asarray(we, np.int32),
                 "label_off": np.asarray(label_off, np.int64), "labels": np.asarray(labels, np.int32)}, has)

    def restated(self, polish):
        bundles, dropped = [], []
        for c, (name, seq, recs, wins) in enumerate(self.contigs):
            last = {}
            for k, r in enumerate(recs):
                last[r[0]] = k
            ivs = []
            for start, end, lab in (wins or []):
                full = [-2] * len(recs)
                for k, v in enumerate(lab):
                    if v != -2:
                        full[last[recs[k][0]]] = v
                ivs.append((start, end, full))
            b, d = pr.contig_bundles(c, pr.sequence_str(seq), [(pr.sequence_str(self.reads[rd][1]), strand, pos, cigar) for rd, strand, pos, cigar in recs],
                                     pr.merge_intervals(ivs), polish, wins is not None)
            bundles += b
            dropped += d
        return bundles, dropped


@functools.lru_cache(maxsize=None)
def _job():
    return Job()


@functools.lru_cache(maxsize=None)
def _restated(polish):
    return _job().restated(polish)


@functools.lru_cache(maxsize=None)
def _batch():
    from hairsplitter_amd import api
    return api.CvBatch(_job().flat())


@functools.lru_cache(maxsize=None)
def _device(polish):
    from hairsplitter_amd import api
    sr, has = _job().sr()
    return api.polish_inputs(_batch(), sr, polish_everything=polish, contig_has_snps=has)


def _as_restated(res):
    """the arrays of api.polish_inputs as the restatement's bundles"""
    out = []
    for i in range(res["n_bundles"]):
        pieces = []
        for p in range(int(res["piece_off"][i]), int(res["piece_off"][i + 1])):
            pieces.append({"rec": int(res["piece_rec"][p]), "read_start": int(res["piece_read_start"][p]), "read_end": int(res["piece_read_end"][p]),
                           "sam_pos": int(res["piece_sam_pos"][p]), "flags": int(res["piece_flags"][p]),
                           "bases": res["bases"][int(res["base_off"][p]):int(res["base_off"][p + 1])].tobytes().decode(),
                           # (no words for an empty range; the reference's convert_cigar2 makes "0 " of the empty string)
                           "cigar": pr.convert_cigar2(pr.convert_cigar(pr.cigar_words_to_string(res["cigar"][int(res["cig_off"][p]):int(res["cig_off"][p + 1])])))})
        out.append({"contig": int(res["bundle_contig"][i]), "interval": int(res["bundle_interval"][i]), "start": int(res["bundle_start"][i]),
                    "end": int(res["bundle_end"][i]), "group": int(res["bundle_group"][i]), "left": int(res["bundle_left_to_polish"][i]),
                    "right": int(res["bundle_right_to_polish"][i]), "overhang_left": int(res["bundle_overhang_left"][i]),
                    "overhang_right": int(res["bundle_overhang_right"][i]),
                    "to_polish": res["backbone"][int(res["backbone_off"][i]):int(res["backbone_off"][i + 1])].tobytes().decode(), "pieces": pieces})
    return out


def _strip(bundles):
    return [dict(b, pieces=[{k: v for k, v in p.items() if k not in ("cigar_start", "cigar_end")} for p in b["pieces"]]) for b in bundles]


@pytest.mark.parametrize("polish", [False, True])
def test_synthetic_records_against_the_restatement(built, polish):
    want, dropped = _restated(polish)
    res = _device(polish)
    got = _as_restated(res)
    assert len(got) == len(want)
    for g, w in zip(got, _strip(want)):
        where = (w["contig"], w["interval"], w["group"])
        assert [p["rec"] for p in g["pieces"]] == [p["rec"] for p in w["pieces"]], where
        for pg_, pw in zip(g["pieces"], w["pieces"]):
            assert pg_ == pw, (where, _job().contigs[w["contig"]][2][pw["rec"]])
        assert g == w, where
    assert sorted(map(tuple, res["dropped"].tolist())) == sorted(dropped)


def test_synthetic_records_cover_the_cases():
    """the inputs above do hold the cases they are meant to hold (judged on the restatement: runs without looking at the device's result)"""
    job = _job()
    want, dropped = _restated(True)
    pieces = [(b, p) for b in want for p in b["pieces"]]
    lengths = set(len(p["bases"]) for _, p in pieces)
    assert set(PIECE_LENGTHS) <= lengths
    b600 = [b for b in want if b["contig"] == 0]
    assert sorted(set((b["left"], b["right"]) for b in b600)) == [(0, 350), (50, 550), (250, 599), (400, 599)]
    assert any(b["group"] == -1 and not b["pieces"] for b in b600)                        # an interval with no label above -1
    assert any(b["group"] == 2 and b["interval"] == 2 and not b["pieces"] for b in b600)  # a group whose reads are all dropped
    assert any(d[0] == 0 and d[1] == 2 for d in dropped) and any(d[0] == 0 and d[1] == 1 for d in dropped)
    assert any(b["contig"] == 2 and (b["start"], b["end"]) == (0, 300) and len(b["to_polish"]) == 300 for b in want)   # the default interval
    assert any(b["contig"] == 1 and b["end"] == 100 for b in want)                          # an interval that ends at L, on the contig with L < 150
    assert not any(b["contig"] in (3, 4) for b in want)
    read_off = np.concatenate(([0], np.cumsum([len(r[1]) for r in job.reads])))      # reads lie in the batch in this order
    for strand in (True, False):
        res = set()
        for b, p in pieces:
            if b["contig"] == 0 and p["bases"]:
                rd, s, pos, cigar = job.contigs[0][2][p["rec"]]
                if s == strand:      # the address of the first source byte of the piece (the last one on the reverse strand)
                    res.add(int(read_off[rd] + p["read_start"] if s else read_off[rd + 1] - 1 - p["read_start"]) % 16)
        assert res == set(range(16))
    # the 200-op CIGAR is cut in chunk 0, at the chunk boundary (op 64, first char) and in chunk 2
    firsts = set()
    for b, p in pieces:
        rd, s, pos, cigar = job.contigs[b["contig"]][2][p["rec"]]
        if b["contig"] == 0 and cigar == LONG:
            ops, at = pr.convert_cigar(cigar), 0
            starts = []
            for w in _cigar_words(cigar):
                starts.append(at)
                at += int(w) >> 4
            firsts.add(max(i for i, s0 in enumerate(starts) if s0 <= p["cigar_start"]) >> 6)
            if p["cigar_start"] == starts[64]:
                firsts.add("op64")
    assert {0, 1, 2, "op64"} <= firsts


def test_start_beyond_the_read_is_flagged(built):
    """posOnReadStart beyond the read: the reference's substr throws (:459); the product returns an empty piece with the flag bit.
    The batch only takes a CIGAR that runs past its read where the alignment runs past the contig end, so that is the record."""
    from hairsplitter_amd import api, synth
    rng = random.Random(3)
    code = {c: i for i, c in enumerate("ACGT")}
    seq, reads = _rand_seq(rng, 600), [_rand_seq(rng, 10), _rand_seq(rng, 10), _rand_seq(rng, 80)]
    recs = [(0, True, 590, "50S20M"), (1, False, 590, "50S20M"), (2, True, 500, "80M")]
    ctg = synth.ContigData("c", np.asarray([code[c] for c in seq], np.uint8), [np.asarray([code[c] for c in r], np.uint8) for r in reads], ["a", "b", "c"],
                           [synth.Alignment(rd, pos, strand, _cigar_words(cg), 0) for rd, strand, pos, cg in recs], np.zeros(3, np.int32))
    batch = api.CvBatch(api.FlatBatch([ctg]))
    sr = {"win_off": np.zeros(2, np.int64), "win_start": np.zeros(0, np.int32), "win_end": np.zeros(0, np.int32), "label_off": np.zeros(1, np.int64),
          "labels": np.zeros(0, np.int32)}
    res = api.polish_inputs(batch, sr, polish_everything=True)
    want, dropped = pr.contig_bundles(0, seq, [(reads[rd], strand, pos, cg) for rd, strand, pos, cg in recs], [], True, has_partitions=False)
    assert _as_restated(res) == _strip(want) and not dropped
    assert res["piece_flags"].tolist() == [api.POLISH_START_BEYOND_SEQ, api.POLISH_START_BEYOND_SEQ, 0]
    assert res["base_off"].tolist() == [0, 0, 0, 80]
    batch.close()


# ---- 3. plumbing --------------------------------------------------------------------------------------
@pytest.mark.parametrize("polish", [0, 1])
def test_tool_file_equals_the_api_result(built, polish):
    """bin/hs_polish_inputs on the job as files (N and lower case in reads and contigs) == api.polish_inputs on it as arrays"""
    from hairsplitter_amd import api
    job = _job()
    res = _device(bool(polish))
    with tempfile.TemporaryDirectory() as td:
        gfa, reads, sam, gro = job.write(td)
        out = os.path.join(td, "polish.txt")
        r = subprocess.run([built["polish_inputs"], gfa, reads, sam, gro, str(polish), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        text = "".join(api.polish_bundle_text(res, i, job.contigs[int(res["bundle_contig"][i])][0]) for i in range(res["n_bundles"]))
        assert open(out).read() == text
        paths = api.polish_bundle_files(res, 0, td)
        assert open(paths["unpolished"]).read().startswith(">seq\n") and open(paths["mapped"]).read().count("\nread") == open(paths["reads"]).read().count(">read")


_ARRAYS = ("bundle_contig", "bundle_interval", "bundle_start", "bundle_end", "bundle_group", "bundle_left_to_polish", "bundle_right_to_polish",
           "bundle_overhang_left", "bundle_overhang_right", "piece_rec", "piece_read_start", "piece_read_end", "piece_sam_pos", "piece_flags")


def _same(a, b):
    for k in _ARRAYS + ("backbone_off", "piece_off", "base_off", "cig_off", "backbone", "bases", "cigar", "dropped"):
        assert np.array_equal(a[k], b[k]), k


def test_split_call_equals_the_unsplit_call(built, monkeypatch):
    from hairsplitter_amd import api
    job = Job(seed=11, big=True)
    batch = api.CvBatch(job.flat())
    sr, has = job.sr()
    whole = api.polish_inputs(batch, sr, polish_everything=True, contig_has_snps=has)
    assert whole["stats"]["n_rounds"] == 1 and whole["base_off"][-1] > 1 << 20
    monkeypatch.setenv("HS_POLISH_CHUNK_MB", "1")
    split = api.polish_inputs(batch, sr, polish_everything=True, contig_has_snps=has)
    assert split["stats"]["n_rounds"] > 1
    _same(whole, split)
    want, dropped = job.restated(True)
    assert _as_restated(split) == _strip(want)
    batch.close()


def test_contig_ranges_concatenate(built):
    from hairsplitter_amd import api
    sr, has = _job().sr()
    whole = _device(True)
    parts = [api.polish_inputs(_batch(), sr, polish_everything=True, c0=a, c1=b, contig_has_snps=has) for a, b in ((0, 1), (1, 1), (1, 3), (3, 5))]
    assert sum(p["n_bundles"] for p in parts) == whole["n_bundles"]
    got = [b for p in parts for b in _as_restated(p)]
    assert got == _as_restated(whole)
    assert np.array_equal(np.concatenate([p["dropped"] for p in parts]), whole["dropped"])
