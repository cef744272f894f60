"""The split mapper on the device (k_map_vote_split and its wide twin through hs_map_reads_split, hs_map_split_to_batch, hs_map_segments_text, HS_MAP_SPLIT)
against the host rule (hs_map_host.cpp through tests/harness/map_split_selftest.cpp) and its numpy form (tests/map_split_cases.py), by integer equality of
every field. tests/test_cpu_map_split.py proves that the two forms agree and that every case reaches the fork it is named after. Every device result is
computed twice: the order inside an index bucket differs from run to run and nothing may depend on it."""
import os
import subprocess

import numpy as np
import pytest

import map_cases as mc
import map_split_cases as sc

pytestmark = pytest.mark.gpu
FIELDS = sc.SEG_FIELDS + sc.READ_FIELDS + ("seg_off",)
RECORD_KEYS = ("contig_rec_off", "rec_interval", "rec_read", "rec_pos", "rec_dist", "rec_strand", "rec_cig_off", "cigar", "dropped")
RUN_KEYS = ("snp_off", "snp_pos", "snp_ref", "snp_alt", "col_off", "col_idx", "col_code", "mean_distance", "depth")


def _device(api, p, sp, contigs, reads):
    """two runs over an index each; the second must equal the first"""
    runs = []
    for _ in range(2):
        with api.map_index(contigs, api.map_params(**p)) as ix:
            runs.append(api.map_reads_split(ix, reads, api.map_split_params(**sp)))
    for k in FIELDS + ("n_wide", "total_minimizers", "total_hits"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    return runs[0]


def _check(api, built, p, sp, contigs, reads, want):
    host = sc.run_harness(built["map_split_selftest"], p, sp, contigs, reads)
    assert host["returncode"] == 0, host
    got = _device(api, p, sp, contigs, reads)
    assert sc.differences(want, got) == [] and sc.differences(host, got) == []
    assert got["n_wide"] == sc.n_wide(want)
    assert got["total_minimizers"] == int(want["n_minimizers"].sum()) and got["total_hits"] == int(want["n_hits"].sum())
    assert api.map_segments_text(got, [len(r) for r in reads], [len(c) for c in contigs]) == host["text"] == sc.paf(want, contigs, reads)
    return got


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_device_equals_the_host_rule(built, name):
    """error-free reads over one cut and over two; one key in two gaps, and a tie between them; a foreign insert, max_gap | max_gap + 1 between two spans;
    max_segments 2 and 8 with a part left over; a second part at min_span - 1 | min_span and at min_votes - 1 | min_votes; a candidate that ends the rounds;
    a k-mer one base into a span; hits at the LDS capacity and above it, each with a second segment"""
    from hairsplitter_amd import api
    p, sp, contigs, reads = sc.get(name)
    got = _check(api, built, p, sp, contigs, reads, sc.want(name))
    with api.map_index(contigs, api.map_params(**p)) as ix:      # a read with one segment has hs_map_reads' record, field for field
        plain = api.map_reads(ix, reads)
    one = np.flatnonzero(np.diff(got["seg_off"]) == 1)
    s = got["seg_off"][one]
    for f in ("contig", "strand", "qstart", "qend", "tstart", "tend", "votes", "second"):
        assert np.array_equal(np.asarray(got[f])[s], plain[f][one]), f
    for f, g in (("n_minimizers", "n_minimizers"), ("n_hits", "n_hits"), ("n_skipped", "n_skipped"), ("votes", "read_votes"), ("second", "read_second")):
        assert np.array_equal(plain[f], got[g]), f
    assert plain["n_wide"] == got["n_wide"]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_one_segment_is_the_plain_mapper(built, name):
    """max_segments = 1 on every case of map_cases: every field of map_cases.FIELDS as the plain rule has it, and as hs_map_reads returns it"""
    from hairsplitter_amd import api
    p, contigs, reads = mc.get(name)
    sp = sc.split(max_segments=1)
    got = _check(api, built, p, sp, contigs, reads, sc.split_numpy(p, sp, contigs, reads))
    one = sc.as_map_result(got)
    with api.map_index(contigs, api.map_params(**p)) as ix:
        plain = api.map_reads(ix, reads)
    for f in mc.FIELDS:
        assert np.array_equal(one[f], mc.want(name)[f]) and np.array_equal(one[f], np.asarray(plain[f], np.int64)), f


def test_noisy_reads_over_a_cut(built):
    """the noisy reads with their contig cut at 5 000 (tests/test_cpu_map_split.py checks the numpy form against the truth): device = host = numpy"""
    from hairsplitter_amd import api
    c, p, sp, contigs = sc.noisy()
    got = _check(api, built, p, sp, contigs, c.reads, sc.split_numpy(p, sp, contigs, c.reads))
    assert int((np.diff(got["seg_off"]) == 2).sum()) >= 20


def test_a_split_call_waits_three_times(built):
    """a count the code defines (hs_capi_map.inc), no measurement: the minimizer total, the hit total with the largest read, and one shipment that carries the
    per-read block, the offsets and as many segments as the device counted -- no wait for their number"""
    from hairsplitter_amd import api
    p, sp, contigs, reads = sc.get("junction_exact")
    with api.map_index(contigs, api.map_params(**p)) as ix:
        api.map_reads_split(ix, reads)      # warm-up: the pools' blocks, the code object
        n0 = api.host_waits()
        res = api.map_reads_split(ix, reads, api.map_split_params(**sp))
        n1 = api.host_waits()
        api.map_reads(ix, reads)
        n2 = api.host_waits()
        api.map_reads_split(ix, [])
        n3 = api.host_waits()
    assert (n1 - n0, n2 - n1) == (3, 3) and n3 - n2 <= 3 and int((np.diff(res["seg_off"]) > 1).sum()) >= 14


def test_bad_parameters_are_refused(built):
    from hairsplitter_amd import api
    with api.map_index([np.zeros(40, np.uint8)]) as ix:
        for bad in (dict(max_segments=0), dict(max_segments=9), dict(min_votes=0), dict(min_span=-1), dict(max_gap=-1)):
            with pytest.raises(api.HsError, match="hs_map_reads_split: split parameters out of range"):
                api.map_reads_split(ix, [np.zeros(40, np.uint8)], api.map_split_params(**bad))
    p, sp, contigs, reads = sc.get("enclose")      # offsets that do not fit the segments: refused, not read
    want = sc.want("enclose")
    lens = [len(r) for r in reads], [len(c) for c in contigs]
    assert api.map_segments_text(want, *lens) == sc.paf(want, contigs, reads)
    for seg_off in ([0, 3, 7], [1, 3, 6], [0, 7, 6]):      # not the segments' number at the end; not 0 in front; not ascending
        with pytest.raises(api.HsError):
            api.map_segments_text(dict(want, seg_off=np.array(seg_off, np.int64)), *lens)


def _seqs(api, contigs, reads):
    cseq, coff = api._flat(contigs)
    rseq, roff = api._flat(reads)
    return dict(contig_seq=cseq, contig_off=coff, read_seq=rseq, read_off=roff)


def test_error_free_reads_over_a_cut_and_the_batch_is_the_truth_batch(built):
    """no tolerance: every read comes back as exactly its parts; the records of hs_map_split_to_batch (contig, read, pos, strand, distance 0, CIGAR words
    [clip S] M [clip S]) equal those of hs_realign_intervals on the truth intervals; every read base is aligned, which the plain mapper cannot give; the
    batch computes what the truth batch computes"""
    from hairsplitter_amd import api
    p, sp, contigs, reads = sc.get("junction_exact")
    truth = [x for parts in sc.junction_truth() for x in parts]
    seqs = _seqs(api, contigs, reads)
    with api.map_index((seqs["contig_seq"], seqs["contig_off"]), api.map_params(**p)) as ix:
        batch, rec, res = api.map_split_to_batch(ix, (seqs["read_seq"], seqs["read_off"]), api.map_split_params(**sp))
        plain, _, _ = api.map_to_batch(ix, (seqs["read_seq"], seqs["read_off"]))
    assert sc.rows(res) == truth
    rec_t, batch_t = api.realign_intervals(seqs, np.array(truth, np.int64))
    assert rec["n_dropped"] == 0 and rec["n_rec"] == len(truth)
    for k in RECORD_KEYS:
        assert np.array_equal(rec[k], rec_t[k]), k
    t = np.array(truth, np.int64)[rec["rec_interval"]]
    assert np.array_equal(rec["rec_read"], t[:, 0]) and np.array_equal(rec["rec_pos"], t[:, 5]) and np.array_equal(rec["rec_strand"], t[:, 2]) and (rec["rec_dist"] == 0).all()
    assert np.array_equal(np.repeat(np.arange(len(contigs)), np.diff(rec["contig_rec_off"])), t[:, 1])
    for i in range(rec["n_rec"]):      # soft clips around one M of the part's length; the clips are the read's other parts (on the contig's strand)
        words = rec["cigar"][rec["rec_cig_off"][i]:rec["rec_cig_off"][i + 1]].tolist()
        Lr, (qs, qe, fwd) = len(reads[t[i, 0]]), (t[i, 3], t[i, 4], t[i, 2])
        left, right = (qs, Lr - qe) if fwd else (Lr - qe, qs)
        assert words == [(n << 4) | op for n, op in ((left, 4), (qe - qs, 0), (right, 4)) if n], (i, words)
    total = sum(len(r) for r in reads)
    assert batch.aligned_bp == batch_t.aligned_bp == total > plain.aligned_bp > 0
    ra, rb = batch.run(), batch_t.run()
    batch.close(); batch_t.close(); plain.close()
    for k in RUN_KEYS:
        assert np.array_equal(ra[k], rb[k]), k


def test_one_read_twice_on_a_contig(built):
    """plumbing: enclose's reads have two segments on one contig each (what a supplementary SAM line gives the reference); the batch equals the one
    hs_realign_intervals makes from the same intervals"""
    from hairsplitter_amd import api
    p, sp, contigs, reads = sc.get("enclose")
    seqs = _seqs(api, contigs, reads)
    with api.map_index((seqs["contig_seq"], seqs["contig_off"]), api.map_params(**p)) as ix:
        batch, rec, res = api.map_split_to_batch(ix, (seqs["read_seq"], seqs["read_off"]), api.map_split_params(**sp))
    assert res["contig"].tolist() == [0, 1, 0, 0, 1, 0] and np.array_equal(api.map_segment_intervals(res), np.array(sc.rows(sc.want("enclose")), np.int64))
    rec2, batch2 = api.realign_intervals(seqs, api.map_segment_intervals(res))
    assert rec["n_rec"] == rec2["n_rec"] == 6 and rec["n_dropped"] == 0
    for k in RECORD_KEYS:
        assert np.array_equal(rec[k], rec2[k]), k
    assert batch.aligned_bp == batch2.aligned_bp > 0
    ra, rb = batch.run(), batch2.run()
    batch.close(); batch2.close()
    for k in RUN_KEYS:
        assert np.array_equal(ra[k], rb[k]), k


def _files(synth, contigs, reads, td):
    cds = [synth.ContigData("piece%d" % i, c, reads if i == 0 else [], ["read%d" % j for j in range(len(reads))] if i == 0 else [], [], np.zeros(0, np.int32)) for i, c in enumerate(contigs)]
    return synth.write_files(cds, td), ["read%d" % j for j in range(len(reads))], [cd.name for cd in cds]


def test_segment_text_goes_through_the_realign_parser(built, tmp_path):
    """hs_map_segments_text's lines (sg / ns tags behind s1 / s2) are PAF lines hs_cv_batch_create_paf accepts, one record per line: the batch of
    hs_map_split_to_batch"""
    from hairsplitter_amd import api, synth
    p, sp, contigs, reads = sc.get("junction_exact")
    f, rn, cn = _files(synth, contigs, reads, str(tmp_path))
    seqs = _seqs(api, contigs, reads)
    with api.map_index((seqs["contig_seq"], seqs["contig_off"]), api.map_params(**p)) as ix:
        batch, rec, res = api.map_split_to_batch(ix, (seqs["read_seq"], seqs["read_off"]), api.map_split_params(**sp))
    text = api.map_segments_text(res, [len(r) for r in reads], [len(c) for c in contigs], rn, cn)
    lines = [l.split("\t") for l in text.splitlines()]
    assert len(lines) == len(res["read"]) and all(len(l) == 16 and l[11] == "255" for l in lines)
    assert [l[14] for l in lines] == ["sg:i:%d" % x for x in res["round"]] and [l[15] for l in lines] == ["ns:i:%d" % x for x in np.repeat(np.diff(res["seg_off"]), np.diff(res["seg_off"]))]
    paf = os.path.join(str(tmp_path), "split.paf")
    open(paf, "w").write(text)
    other = api.CvBatch.from_paf(f["gfa"], f["reads"], paf)
    assert other.records["n_rec"] == rec["n_rec"]
    for k in ("rec_read", "rec_pos", "rec_strand", "cigar", "contig_rec_off"):
        assert np.array_equal(other.records[k], rec[k]), k
    assert other.aligned_bp == batch.aligned_bp
    other.close(); batch.close()


def test_the_tool_and_the_drop_in_take_the_switch(built, tmp_path):
    """bin/hs_map with HS_MAP_SPLIT=4 writes hs_map_segments_text's lines; that PAF through HS_REALIGN=1 HS_call_variants gives the .col and the error rate of
    HS_MAP=1 HS_MAP_SPLIT=4 HS_call_variants; without the switch, or with 1, the tool writes hs_map_text's bytes, and so it does, with a line on stderr, at 9"""
    from hairsplitter_amd import api, synth
    td = str(tmp_path)
    c, p, sp, contigs = sc.noisy()
    f, rn, cn = _files(synth, contigs, c.reads, td)
    with api.map_index(contigs) as ix:
        seg = api.map_reads_split(ix, c.reads, api.map_split_params(max_segments=4))
        plain = api.map_reads(ix, c.reads)
    lens = [len(r) for r in c.reads], [len(x) for x in contigs]
    want_split, want_plain = api.map_segments_text(seg, lens[0], lens[1], rn, cn), api.map_text(plain, lens[0], lens[1], rn, cn)
    assert len(want_split.splitlines()) >= len(want_plain.splitlines()) + 20
    env = {k: v for k, v in os.environ.items() if k != "HS_MAP_SPLIT"}
    texts = {}
    for tag, extra in (("split", {"HS_MAP_SPLIT": "4"}), ("unset", {}), ("one", {"HS_MAP_SPLIT": "1"}), ("nine", {"HS_MAP_SPLIT": "9"})):
        out = os.path.join(td, tag + ".paf")
        r = subprocess.run([built["map"], f["gfa"], f["reads"], out, "4"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(env, **extra))
        texts[tag] = open(out).read()
        assert (b"HS_MAP_SPLIT=9 is not one of 1..8" in r.stderr) == (tag == "nine")      # a value the switch does not take is named, not dropped in silence
    assert texts["split"] == want_split and texts["unset"] == want_plain and texts["one"] == want_plain and texts["nine"] == want_plain
    cols = {}
    for tag, aln, extra in (("paf", os.path.join(td, "split.paf"), {"HS_REALIGN": "1"}), ("map", os.path.join(td, "not_there.sam"), {"HS_MAP": "1", "HS_MAP_SPLIT": "4"}),
                            ("plain", os.path.join(td, "not_there.sam"), {"HS_MAP": "1"})):
        col, vcf, err = (os.path.join(td, tag + x) for x in (".col", ".vcf", ".err"))
        subprocess.run([built["cv"], f["gfa"], f["reads"], aln, "2", td, err, "0", "0", col, vcf, "0.33"], check=True, stdout=subprocess.DEVNULL,
                       env=dict(env, HS_NO_PRECOMPUTE="1", **extra))
        cols[tag] = (open(col, "rb").read(), open(err).read())
    assert cols["paf"] == cols["map"] and len(cols["map"][0]) > 1000
    assert cols["map"][0] != cols["plain"][0]      # the reads over the cut now count on both pieces
