"""Anchored alignment on the device (k_map_anchors behind the vote through hs_map_reads_anchored; k_anchor_join_plan / k_anchor_join through
hs_realign_intervals_anchored; hs_map_to_batch_anchored) against the host rule (tests/harness/map_anchor_selftest.cpp), its numpy form and the stitched
expectation of tests/anchor_cases.py, by integer equality. tests/test_cpu_map_anchors.py proves that the two forms of the rule agree and that every case
reaches its fork. Every mapper result is computed twice: the order inside an index bucket differs from run to run and nothing may depend on it."""
import numpy as np
import pytest

import anchor_cases as ac
import map_cases as mc

pytestmark = pytest.mark.gpu
PAD = 100


# ---- 1. device = host = numpy ----
def _device(api, p, spacing, contigs, reads):
    runs = []
    for _ in range(2):
        with api.map_index(contigs, api.map_params(**p)) as ix:
            res, anc = api.map_reads_anchored(ix, reads, api.map_anchor_params(spacing=spacing))
            plain = api.map_reads(ix, reads)
        for f in mc.FIELDS:
            assert np.array_equal(res[f], plain[f]), f
        assert (res["n_wide"], res["total_minimizers"], res["total_hits"]) == (plain["n_wide"], plain["total_minimizers"], plain["total_hits"])
        runs.append((res, anc))
    assert ac.differences(runs[0][1], runs[1][1]) == []
    return runs[0]


def _check(api, built, p, spacing, contigs, reads, want):
    host = ac.run_harness(built["map_anchor_selftest"], p, spacing, contigs, reads)
    assert host["returncode"] == 0, host
    res, anc = _device(api, p, spacing, contigs, reads)
    assert ac.differences(want, anc) == [] and ac.differences(host, anc) == []
    assert mc.differences(want["map"], res) == []
    assert ac.inside_interval(res, anc, reads)
    return res, anc


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_device_equals_the_host_rule(built, name):
    """both strands; unmapped reads; hits at the LDS capacity (anchors) and one above it (none); a chain that leaves a member out of the cuts"""
    from hairsplitter_amd import api
    p, spacing, contigs, reads = ac.get(name)
    res, anc = _check(api, built, p, spacing, contigs, reads, ac.want(name))
    if name == "capacity":
        assert res["n_wide"] == 1 and anc["n_best"][0] > 0 and anc["n_best"][1] == 0


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_every_case_of_the_mapper(built, name):
    from hairsplitter_amd import api
    p, contigs, reads = mc.get(name)
    _check(api, built, p, 64, contigs, reads, ac.want_map_case(name))


@pytest.mark.parametrize("spacing", [1, 256])
def test_noisy_reads(built, spacing):
    """310 noisy reads: the ordered hits of every one rise strictly in t, so the chain is all of them (the fast path; counted from the numpy form); at
    spacing 1 every supported member is a cut"""
    from hairsplitter_amd import api
    c, p, contigs, want = ac.noisy(spacing)
    _, anc = _check(api, built, p, spacing, contigs, c.reads, want)
    assert all(d["n_chain"] == d["n_best"] for d in want["detail"]) and (np.diff(anc["anc_off"]) >= 1).all()
    if spacing == 1:
        assert np.array_equal(np.diff(anc["anc_off"]), anc["n_supported"])


def test_a_chain_that_is_not_every_hit(built):
    """the patience pass on the device: a homopolymer and a dinucleotide run give hundreds of hits that fall in t, most of them off the chain; the read at
    the LDS capacity keeps half of the best's; lone_seed leaves one member without support. (The fast path: every noisy read, test_noisy_reads.)"""
    from hairsplitter_amd import api
    w = ac.want("lone_seed")
    assert w["n_chain"][0] < w["n_best"][0] and w["n_supported"][0] < w["n_chain"][0]
    want = ac.want_map_case("homopolymer")
    assert (want["n_chain"][[1, 3]] * 10 < want["n_best"][[1, 3]]).all() and (want["n_chain"][[1, 3]] >= 10).all()
    want = ac.want_map_case("capacity")
    assert 0 < want["n_chain"][0] < want["n_best"][0]
    for name in ("homopolymer", "capacity"):
        p, contigs, reads = mc.get(name)
        _check(api, built, p, 64, contigs, reads, ac.want_map_case(name))


def test_an_anchored_call_waits_three_times(built):
    """a count the code defines (hs_capi_map.inc): the minimizer total, the hit total, and one shipment that carries the per-read block, the anchor offsets
    and as many anchors as the device counted"""
    from hairsplitter_amd import api
    p, spacing, contigs, reads = ac.get("strands")
    with api.map_index(contigs, api.map_params(**p)) as ix:
        api.map_reads_anchored(ix, reads)      # warm-up: the pools' blocks, the code object
        n0 = api.host_waits()
        _, anc = api.map_reads_anchored(ix, reads, api.map_anchor_params(spacing=spacing))
        n1 = api.host_waits()
        api.map_reads(ix, reads)
        n2 = api.host_waits()
    assert (n1 - n0, n2 - n1) == (3, 3) and len(anc["anc_q"]) >= 10


def test_bad_parameters_are_refused(built):
    from hairsplitter_amd import api
    with api.map_index([np.zeros(40, np.uint8)]) as ix:
        with pytest.raises(api.HsError, match="hs_map_reads_anchored: anchor parameters out of range"):
            api.map_reads_anchored(ix, [np.zeros(40, np.uint8)], api.map_anchor_params(spacing=0))
    assert api.map_anchor_params().spacing >= 1


# ---- 2. explicit anchors ----
def _mutated(g, seq, n_sub, indels):
    """`seq` with n_sub substitutions and the given indels ((position, +n inserted | -n deleted), positions ascending)"""
    s = np.array(seq, np.uint8)
    at = g.choice(len(s), size=n_sub, replace=False) if n_sub else []
    s[at] = (s[at] + 1 + g.integers(0, 3, size=len(at))) & 3
    out, last = [], 0
    for pos, n in indels:
        out.append(s[last:pos])
        if n > 0:
            out.append(mc._rand(g, n))
        last = pos - min(n, 0)
    return np.concatenate(out + [s[last:]])


@pytest.fixture(scope="module")
def job():
    """one contig of 9 000 bases and the reads of every shape; per interval its anchors as (q, t) on the read as it aligns"""
    g = np.random.default_rng([0x414A, 1])
    C = mc._rand(g, 9000)
    reads, ivs, ancs, names = [], [], [], []

    def add(name, start, L, strand, anchors, n_sub=4, indels=(), lead=0, trail=0, read=None):
        """a read cut from C[start, start + L) with errors (lead / trail: foreign bases in front / behind, inside the interval); anchors relative to
        (a0, tstart)"""
        if read is None:
            body = _mutated(g, C[start:start + L], n_sub, indels)
            read = np.concatenate([mc._rand(g, lead), body, mc._rand(g, trail)])
        Lr = len(read)
        reads.append(read if strand else mc.rc(read))
        ivs.append((len(reads) - 1, 0, strand, 0, Lr, start, start + L))
        ancs.append([(q, start + t) for q, t in anchors])
        names.append(name)

    for st in (1, 0):
        add("none", 1000, 300, st, [], indels=((100, 2), (200, -3)))
        add("anchor_at_a0", 1400, 200, st, [(0, 0)])
        add("anchor_at_a1", 1700, 200, st, [(200, 200)])
        add("tail_of_one_base", 2000, 120, st, [(60, 60), (119, 119)])
        add("neighbours", 2200, 150, st, [(50, 50), (51, 51), (52, 52), (100, 100)])
        add("skew_neighbours", 2400, 150, st, [(40, 40), (41, 45), (46, 46), (100, 100)], n_sub=0)
        add("indels_between", 2600, 600, st, [(20, 20), (300, 297), (580, 581)], indels=((150, -3), (400, 4)))
        add("forty", 3300, 40, st, [(20, 20)], n_sub=1)
    add("contig_start_empty_head_target", 0, 200, 1, [(6, 0), (100, 94)], n_sub=2, lead=6)
    add("contig_start_minus", 0, 200, 0, [(6, 0), (100, 94)], n_sub=2, lead=6)
    add("contig_end_empty_tail_target", 8800, 200, 1, [(100, 100), (200, 200)], n_sub=2, trail=7)
    add("overhang", 8700, 300, 0, [(50, 50), (250, 250)], n_sub=3, trail=40)
    add("middle_2048", 4000, 2200, 1, [(10, 10), (2058, 2058)], n_sub=20)
    add("middle_2049", 4000, 2200, 0, [(10, 10), (2059, 2059)], n_sub=20)
    add("head_1100", 6300, 1300, 1, [(1100, 1101)], n_sub=12, indels=((300, 1), (700, -2)))
    add("head_1100_minus", 6300, 1300, 0, [(1100, 1101)], n_sub=12, indels=((300, 1), (700, -2)))
    # two intervals of one read
    two = np.concatenate([C[500:800], C[7700:8000]])
    reads.append(two)
    for k, (qs, ts) in enumerate(((0, 500), (300, 7700))):
        ivs.append((len(reads) - 1, 0, 1, qs, qs + 300, ts, ts + 300))
        ancs.append([(qs + 100, ts + 100), (qs + 200, ts + 200)])
        names.append("two_intervals_%d" % k)
    off = np.concatenate([[0], np.cumsum([len(a) for a in ancs])]).astype(np.int64)
    flat = dict(contig_seq=C, contig_off=np.array([0, len(C)], np.int64), read_seq=np.concatenate(reads),
                read_off=np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64))
    aq = np.array([q for a in ancs for q, _ in a], np.int32)
    at = np.array([t for a in ancs for _, t in a], np.int32)
    return dict(C=C, reads=reads, ivs=np.array(ivs, np.int64), ancs=ancs, names=names, flat=flat, off=off, aq=aq, at=at)


def _expected(api, job):
    return ac.expected_records(api, job, PAD)


def _records(rec):
    """record of every interval: (pos, NM, strand, words)"""
    return {int(i): (int(rec["rec_pos"][k]), int(rec["rec_dist"][k]), int(rec["rec_strand"][k]), rec["cigar"][rec["rec_cig_off"][k]:rec["rec_cig_off"][k + 1]])
            for k, i in enumerate(rec["rec_interval"])}


def _walk_holds(rec, ivs, reads, contigs, pad):
    """every record's CIGAR consumes exactly its read, stays inside the interval's window and counts NM edits"""
    for i, (pos, nm, strand, words) in _records(rec).items():
        iv = ivs[i]
        read, contig = reads[iv[0]], contigs[iv[1]]
        got = ac.walk_cigar(words, pos, read, contig, int(iv[2]), ac.window_of(len(contig), int(iv[5]), int(iv[6]), pad))
        assert got == (len(read), nm, True) and strand == int(iv[2]), (i, got, len(read), nm)


def test_explicit_anchors(built, job):
    """no anchors, an anchor at either end of the read range, a tail of one base, pieces of 1 x 1, 1 x 5 and 5 x 1, indels between anchors, an interval of
    40 bases, an empty head target at contig position 0 and an empty tail target at the contig's end (runs of insertions), a read that overhangs the contig, a
    middle of 2 048 | 2 049 query bases (the grouped | wavefront kernels of A1), a head of more than 1 024 moves read backwards, two intervals of one read;
    both strands. Words, pos, NM and strand equal the stitched pieces'; the CIGAR walk holds on every record."""
    from hairsplitter_amd import api
    rec, _ = api.realign_intervals_anchored(job["flat"], job["ivs"], job["off"], job["aq"], job["at"], pad=PAD, want_batch=False)
    want = _expected(api, job)
    got = _records(rec)
    assert rec["n_dropped"] == 0 and sorted(got) == list(range(len(job["ivs"])))
    for i, w in enumerate(want):
        pos, nm, strand, words = got[i]
        assert (pos, nm, strand) == (w["pos"], w["nm"], int(job["ivs"][i][2])) and np.array_equal(words, w["words"]), (job["names"][i], got[i], w)
    assert rec["n_pieces"] == sum(w["n_pieces"] for w in want)
    _walk_holds(rec, job["ivs"], job["reads"], [job["C"]], PAD)
    # the shapes are what their names say
    pcs = {n: ac.pieces_of(iv, len(job["reads"][iv[0]]), len(job["C"]), [q for q, _ in a], [t for _, t in a], PAD)[0] for n, iv, a in zip(job["names"], job["ivs"], job["ancs"])}
    assert [p[0] for p in pcs["contig_start_empty_head_target"]] == ["INS", "MID", "TAIL"] and [p[0] for p in pcs["contig_end_empty_tail_target"]][-1] == "INS"
    assert [p[0] for p in pcs["anchor_at_a0"]] == ["TAIL"] and [p[0] for p in pcs["anchor_at_a1"]] == ["HEAD"]
    assert pcs["middle_2048"][1][2] - pcs["middle_2048"][1][1] == 2048 and pcs["middle_2049"][1][2] - pcs["middle_2049"][1][1] == 2049
    assert pcs["tail_of_one_base"][-1][2] - pcs["tail_of_one_base"][-1][1] == 1
    assert all(pcs[n][0][0] == "HEAD" and pcs[n][0][2] - pcs[n][0][1] == 1100 > 1024 for n in ("head_1100", "head_1100_minus"))


def test_no_anchors_is_the_plain_route(built, job):
    """without anchors the records equal hs_realign_intervals' records word for word"""
    from hairsplitter_amd import api
    none = np.zeros(len(job["ivs"]) + 1, np.int64)
    a, _ = api.realign_intervals_anchored(job["flat"], job["ivs"], none, [], [], pad=PAD, want_batch=False)
    b, _ = api.realign_intervals(job["flat"], job["ivs"], pad=PAD, want_batch=False)
    for k in ("contig_rec_off", "rec_interval", "rec_read", "rec_pos", "rec_dist", "rec_strand", "rec_cig_off", "cigar", "dropped"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_pieces"] == b["n_pieces"] == len(job["ivs"])


def test_anchored_never_beats_the_plain_route(built, job):
    """NM(anchored) >= NM(plain) on every interval: an alignment through the anchors is a feasible HW alignment in the same window"""
    from hairsplitter_amd import api
    a, _ = api.realign_intervals_anchored(job["flat"], job["ivs"], job["off"], job["aq"], job["at"], pad=PAD, want_batch=False)
    b, _ = api.realign_intervals(job["flat"], job["ivs"], pad=PAD, want_batch=False)
    ra, rb = _records(a), _records(b)
    assert all(ra[i][1] >= rb[i][1] for i in ra) and sorted(ra) == sorted(rb)


def test_invalid_anchors_are_refused(built, job):
    from hairsplitter_amd import api
    i = job["names"].index("neighbours")
    iv = job["ivs"][i:i + 1]
    t0 = int(iv[0][5])
    for bad in ([(50, t0 + 50), (50, t0 + 60)], [(50, t0 + 50), (60, t0 + 50)], [(60, t0 + 60), (50, t0 + 50)], [(-1, t0)], [(10, t0 - 1)], [(10, t0 + 151)], [(1000, t0 + 20)]):
        with pytest.raises(api.HsError, match="hs_realign_intervals_anchored: interval 0: anchor"):
            api.realign_intervals_anchored(job["flat"], iv, [0, len(bad)], [q for q, _ in bad], [t for _, t in bad], pad=PAD, want_batch=False)


# ---- 3. error-free reads ----
def test_error_free_reads(built):
    """map_cases.exact_reads through hs_map_to_batch_anchored: every read's record is its truth, distance 0 and one run of Lr matches"""
    from hairsplitter_amd import api
    p, c, reads, starts, strands = mc.exact_reads()
    with api.map_index([c], api.map_params(**p)) as ix:
        batch, rec, res, anc = api.map_to_batch_anchored(ix, reads, api.map_anchor_params(spacing=64), pad=PAD)
        batch.close()
    got = _records(rec)
    mapped = np.flatnonzero(res["contig"] >= 0)
    assert len(mapped) == len(reads) and rec["n_dropped"] == 0 and (np.diff(anc["anc_off"]) >= 1).sum() >= 40
    for k, r in enumerate(mapped):
        pos, nm, strand, words = got[k]
        assert (pos, nm, strand) == (starts[r], 0, strands[r]) and words.tolist() == [len(reads[r]) << 4], (r, got[k])


# ---- 4. noisy reads ----
@pytest.fixture(scope="module")
def noisy_plain(built):
    from hairsplitter_amd import api
    c = ac._noisy_case()
    with api.map_index([c.seq], api.map_params(**mc.params())) as ix:
        batch, rec, res = api.map_to_batch(ix, c.reads, pad=PAD)
        run = batch.run()
        batch.close()
    return rec, res, run


@pytest.mark.parametrize("spacing", [128, 256])
def test_noisy_reads_cost_what_the_plain_route_costs(built, noisy_plain, spacing):
    """310 noisy reads: per read NM through the anchors == NM of hs_map_to_batch (the integer condition tests/test_cpu_map_anchors.py holds by a DP of its
    own), the CIGAR walk holds on every record, no read is dropped, n_pieces is the anchors' count. The two batches' stage-3 results are printed, not
    asserted: equally cheap paths may place an indel differently."""
    from hairsplitter_amd import api
    c = ac._noisy_case()
    plain, plain_res, plain_run = noisy_plain
    with api.map_index([c.seq], api.map_params(**mc.params())) as ix:
        batch, rec, res, anc = api.map_to_batch_anchored(ix, c.reads, api.map_anchor_params(spacing=spacing), pad=PAD)
        run = batch.run()
        batch.close()
    for f in mc.FIELDS:
        assert np.array_equal(res[f], plain_res[f]), f
    assert rec["n_dropped"] == 0 and plain["n_dropped"] == 0 and rec["n_rec"] == plain["n_rec"] == len(c.reads) == 310
    a, b = _records(rec), _records(plain)
    above = [i for i in a if a[i][1] != b[i][1]]
    print("spacing %d: sum NM anchored %d plain %d, reads above %d, pieces %d" % (spacing, sum(v[1] for v in a.values()), sum(v[1] for v in b.values()), len(above), rec["n_pieces"]))
    assert above == []
    ivs = api.map_intervals(res)
    _walk_holds(rec, ivs, c.reads, [c.seq], PAD)
    n_anc = np.diff(anc["anc_off"])
    want_pieces = 0
    for i, iv in enumerate(ivs):
        o = int(anc["anc_off"][iv[0]])
        pcs, _, _ = ac.pieces_of(iv, len(c.reads[iv[0]]), len(c.seq), anc["anc_q"][o:o + n_anc[iv[0]]], anc["anc_t"][o:o + n_anc[iv[0]]], PAD)
        want_pieces += sum(p[0] != "INS" for p in pcs)
    assert rec["n_pieces"] == want_pieces
    sa, sb = set(np.asarray(run["snp_pos"]).tolist()), set(np.asarray(plain_run["snp_pos"]).tolist())
    print("spacing %d: SNPs anchored %d plain %d in common %d" % (spacing, len(sa), len(sb), len(sa & sb)))
