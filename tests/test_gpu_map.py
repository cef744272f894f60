"""The read mapper on the device (hs_kernels_map.hip through hs_map_index_create, hs_map_reads, hs_map_to_batch, hs_map_text) against the host rule
(hs_map_host.cpp through tests/harness/map_selftest.cpp) and its numpy form (tests/map_cases.py), by integer equality of every field; the index's
buckets as sorted multisets. tests/test_cpu_map_cases.py proves that the two forms agree and that every case reaches the fork it is named after."""
import os
import subprocess

import numpy as np
import pytest

import map_cases as mc
from test_cpu_map_cases import NAMES, noisy_case, noisy_check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(api, p):
    return api.map_params(**p)


def _device(api, p, contigs, reads):
    with api.map_index(contigs, _params(api, p)) as ix:
        ent = ix.entries()
        res = api.map_reads(ix, reads)
    b = np.repeat(np.arange(len(ent["bucket_off"]) - 1), np.diff(ent["bucket_off"]))
    res["index_rows"] = np.stack([b, ent["hash"].astype(np.int64), ent["contig"].astype(np.int64), ent["t"], ent["strand"].astype(np.int64)], axis=1).reshape(-1, 5)
    res["bucket_bits"] = ent["bucket_bits"]
    return res


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_rule(built, name):
    """lengths 0 .. k + w - 1 and empty calls; k 5 / 15 / 16, w 1 / 10 / 32; equal hashes across a window, windows of palindromes; occ 64 | 65; bin edges, an
    indel over two bins, bins three apart; ties between contigs and strands; both contig ends with and without `extend`; hits at the LDS capacity | + 1 and
    a tandem repeat through the scratch route; one bucket, eight, the default; best = min_votes - 1 | min_votes; error-free reads"""
    from hairsplitter_amd import api
    assert api.map_lds_capacity() == mc.LDS_CAPACITY
    p, contigs, reads = mc.get(name)
    want = mc.want(name)
    host = mc.run_harness(built["map_selftest"], p, contigs, reads)
    assert host["returncode"] == 0, host
    got = _device(api, p, contigs, reads)
    for ref in (want, host):
        ref_fields = {f: ref[f] for f in mc.FIELDS}
        assert [f for f in mc.FIELDS if not np.array_equal(np.asarray(ref_fields[f], np.int64), np.asarray(got[f], np.int64))] == []
    assert mc.differences(want, {k: got[k] for k in mc.FIELDS + ("index_rows", "bucket_bits")}) == []      # (the index: sorted multisets per bucket)
    assert got["n_wide"] == mc.n_wide(want)
    assert got["total_minimizers"] == int(want["n_minimizers"].sum()) and got["total_hits"] == int(want["n_hits"].sum())
    assert api.map_text(got, [len(r) for r in reads], [len(c) for c in contigs]) == host["text"]
    again = _device(api, p, contigs, reads)      # the order inside a bucket may differ from run to run: nothing may depend on it
    for k in mc.FIELDS + ("n_wide",):
        assert np.array_equal(got[k], again[k]), k
    assert np.array_equal(again["index_rows"][np.lexsort(again["index_rows"].T[::-1])], got["index_rows"][np.lexsort(got["index_rows"].T[::-1])])


def test_one_index_serves_many_calls(built):
    from hairsplitter_amd import api
    p, contigs, reads = mc.get("k15_w10")
    want = mc.want("k15_w10")
    with api.map_index(contigs, _params(api, p)) as ix:
        whole = api.map_reads(ix, reads)
        parts = [api.map_reads(ix, reads[:2]), api.map_reads(ix, reads[2:])]
    for f in mc.FIELDS:
        assert np.array_equal(whole[f], want[f]) and np.array_equal(np.concatenate([x[f] for x in parts]), want[f]), f


def test_an_index_call_waits_twice_and_a_map_call_three_times(built):
    """a count the code defines (hs_capi_map.inc), no measurement: the minimizer total and the end for an index; the minimizer total, the hit total with
    the largest read, and the records' one shipment for a map call. A call without a base has no minimizers to wait for."""
    from hairsplitter_amd import api
    p, contigs, reads = mc.get("k15_w10")
    with api.map_index(contigs, _params(api, p)) as ix:      # warm-up: the pools' blocks, the code object
        api.map_reads(ix, reads)
    n0 = api.host_waits()
    with api.map_index(contigs, _params(api, p)) as ix:
        n1 = api.host_waits()
        api.map_reads(ix, reads)
        n2 = api.host_waits()
        api.map_reads(ix, [])
        n3 = api.host_waits()
        api.map_reads(ix, [np.zeros(0, np.uint8), np.zeros(0, np.uint8)])
        n4 = api.host_waits()
    assert (n1 - n0, n2 - n1) == (2, 3)
    assert n3 - n2 <= 3 and n4 - n3 <= 3
    p, contigs, reads = mc.get("no_reads")
    with api.map_index(contigs, _params(api, p)) as ix:
        n5 = api.host_waits()
        api.map_reads(ix, reads)
        assert api.host_waits() - n5 <= 3


def test_bad_input_is_refused(built):
    from hairsplitter_amd import api
    for bad in (dict(k=4), dict(k=17), dict(w=0), dict(w=33), dict(bucket_bits=27)):
        with pytest.raises(api.HsError, match="hs_map_index_create: parameters out of range"):
            api.map_index([np.zeros(40, np.uint8)], api.map_params(**bad))
    with api.map_index([np.zeros(40, np.uint8)]) as ix:
        with pytest.raises(api.HsError, match="hs_map_reads: offsets must ascend"):
            api.map_reads(ix, (np.zeros(10, np.uint8), np.array([0, 7, 5], np.int64)))


def _exact_contig():
    from hairsplitter_amd import synth
    p, c, reads, starts, strands = mc.exact_reads()
    alns = [synth.Alignment(i, s, bool(st), np.array([(len(r) << 4) | synth.OP_M], np.uint32), 0) for i, (r, s, st) in enumerate(zip(reads, starts, strands))]
    return p, synth.ContigData("exact", c, reads, ["exact_r%d" % i for i in range(len(reads))], alns, np.zeros(len(reads), np.int32))


def test_error_free_reads_map_to_their_origin_and_the_batch_is_the_truth_batch(built):
    """no tolerance: every read comes back on [s, s + Lr), and the batch of hs_map_to_batch equals the batch made from the truth alignments (pos; one M op)"""
    from hairsplitter_amd import api
    p, cd = _exact_contig()
    flat = api.FlatBatch([cd])
    with api.map_index((flat.contig_seq, flat.contig_off), _params(api, p)) as ix:
        batch, rec, res = api.map_to_batch(ix, (flat.read_seq, flat.read_off))
        alone = api.map_reads(ix, (flat.read_seq, flat.read_off))
    for a in cd.alns:
        i, L = a.read, len(cd.reads[a.read])
        assert (res["contig"][i], res["strand"][i], res["qstart"][i], res["qend"][i], res["tstart"][i], res["tend"][i]) == (0, int(a.strand), 0, L, a.pos, a.pos + L), i
    for f in mc.FIELDS:
        assert np.array_equal(res[f], alone[f]), f
    assert rec["n_dropped"] == 0 and rec["rec_read"].tolist() == list(range(len(cd.reads)))
    assert rec["rec_pos"].tolist() == [a.pos for a in cd.alns] and rec["rec_dist"].tolist() == [0] * len(cd.alns)
    assert rec["cigar"].tolist() == [int(a.cigar[0]) for a in cd.alns]
    truth = api.CvBatch(flat)
    assert batch.aligned_bp == truth.aligned_bp > 0
    ra, rb = batch.run(), truth.run()
    batch.close(); truth.close()
    for k in ("snp_off", "snp_pos", "snp_ref", "snp_alt", "col_off", "col_idx", "col_code", "mean_distance", "depth"):
        assert np.array_equal(ra[k], rb[k]), k


def test_to_batch_is_map_reads_then_realign_intervals(built):
    """plumbing, on noisy reads: the records of hs_map_to_batch equal hs_realign_intervals called with the intervals hs_map_reads returned; the noisy
    reads' windows hold their true spans (the condition tests/test_cpu_map_cases.py checks on the numpy form)"""
    from hairsplitter_amd import api
    cd = noisy_case()
    flat = api.FlatBatch([cd])
    with api.map_index((flat.contig_seq, flat.contig_off)) as ix:
        batch, rec, res = api.map_to_batch(ix, (flat.read_seq, flat.read_off))
        alone = api.map_reads(ix, (flat.read_seq, flat.read_off))
    bp = batch.aligned_bp
    batch.close()
    want = mc.map_numpy(mc.params(), [cd.seq], cd.reads)
    for f in mc.FIELDS:
        assert np.array_equal(res[f], want[f]) and np.array_equal(alone[f], want[f]), f
    noisy_check(cd, res)
    rec2, none = api.realign_intervals(flat, api.map_intervals(alone), want_batch=False)
    assert none is None and bp > 0 and rec["n_rec"] == rec2["n_rec"] > 0
    for k in ("contig_rec_off", "rec_interval", "rec_read", "rec_pos", "rec_dist", "rec_strand", "rec_cig_off", "cigar", "dropped"):
        assert np.array_equal(rec[k], rec2[k]), k


def test_paf_text_goes_through_the_realign_parser(built, tmp_path):
    """hs_map_text's lines (votes, span, 255, s1 / s2 tags) are PAF lines hs_cv_batch_create_paf accepts: the batch equals hs_map_to_batch's"""
    from hairsplitter_amd import api, synth
    cd = noisy_case()
    f = synth.write_files([cd], str(tmp_path))
    flat = api.FlatBatch([cd])
    with api.map_index((flat.contig_seq, flat.contig_off)) as ix:
        batch, rec, res = api.map_to_batch(ix, (flat.read_seq, flat.read_off))
    text = api.map_text(res, [len(r) for r in cd.reads], [len(cd.seq)], cd.read_names, [cd.name])
    lines = text.splitlines()
    assert len(lines) == int((res["contig"] >= 0).sum()) and all(len(l.split("\t")) == 14 and l.split("\t")[11] == "255" for l in lines)
    paf = os.path.join(str(tmp_path), "map.paf")
    open(paf, "w").write(text)
    other = api.CvBatch.from_paf(f["gfa"], f["reads"], paf)
    assert other.records["n_rec"] == rec["n_rec"] and np.array_equal(other.records["rec_pos"], rec["rec_pos"]) and np.array_equal(other.records["cigar"], rec["cigar"])
    assert other.aligned_bp == batch.aligned_bp
    other.close(); batch.close()


def test_the_tool_and_the_drop_in_take_the_same_route(built, tmp_path):
    """bin/hs_map's PAF through HS_REALIGN=1 HS_call_variants gives the .col of HS_MAP=1 HS_call_variants (which does not read its alignment argument);
    an assembly given as FASTA maps like the GFA"""
    from hairsplitter_amd import api, synth
    td = str(tmp_path)
    cd = noisy_case()
    f = synth.write_files([cd], td)
    paf, paf_fa, fasta = (os.path.join(td, x) for x in ("tool.paf", "tool_fa.paf", "assembly.fasta"))
    subprocess.run([built["map"], f["gfa"], f["reads"], paf, "4"], check=True, stdout=subprocess.DEVNULL)
    text = open(paf).read()
    with api.map_index([cd.seq]) as ix:
        res = api.map_reads(ix, cd.reads)
    assert text == api.map_text(res, [len(r) for r in cd.reads], [len(cd.seq)], cd.read_names, [cd.name]) and len(text.splitlines()) > 200
    seq = synth._ACGT[cd.seq].tobytes().decode()
    open(fasta, "w").write(">%s some description\n" % cd.name + "".join(seq[i:i + 70] + "\n" for i in range(0, len(seq), 70)))
    subprocess.run([built["map"], fasta, f["reads"], paf_fa], check=True, stdout=subprocess.DEVNULL)
    assert open(paf_fa).read() == text
    cols = {}
    for tag, aln, env in (("paf", paf, {"HS_REALIGN": "1"}), ("map", os.path.join(td, "not_there.sam"), {"HS_MAP": "1"})):
        col, vcf, err = (os.path.join(td, tag + x) for x in (".col", ".vcf", ".err"))
        subprocess.run([built["cv"], f["gfa"], f["reads"], aln, "2", td, err, "0", "0", col, vcf, "0.33"], check=True, stdout=subprocess.DEVNULL,
                       env=dict(os.environ, HS_NO_PRECOMPUTE="1", **env))
        cols[tag] = (open(col, "rb").read(), open(err).read())
    assert cols["paf"] == cols["map"] and len(cols["map"][0]) > 1000
