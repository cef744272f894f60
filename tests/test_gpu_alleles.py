"""The allele table on the device (hs_kernels_alleles.hip through hs_haplotype_alleles, HS_PIPELINE_ALLELES and HS_ALLELES=1) against the brute-force
statement of the rule in tests/allele_cases.py, by integer equality of every field. tests/test_cpu_allele_cases.py proves that every case reaches the
fork it is named after."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import allele_cases as ac
import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lds_cap(built):
    from hairsplitter_amd import api
    cap = api.alleles_lds_capacity()
    assert 64 < cap < 65535
    return cap


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_device_table_equals_the_rule(built, lds_cap, name):
    """depths: 1 .. 256 entries and the first column past the LDS route; groups: 1 .. 300 groups, sparse ids, a window without groups; codes: every
    branch of the call; labels: -1 / -2 inside a column; windows: borders, empty windows and contigs, col_off != 0; deepest: 65535 entries"""
    from hairsplitter_amd import api
    contigs, sr = ac.get(name, lds_cap)
    got = api.haplotype_alleles(contigs, sr)
    assert ac.differences(ac.rule_brute(contigs, sr), got) == []
    deep = sum(int((np.diff(c["col_off"]) > lds_cap).sum()) for c in contigs)
    assert got["n_wide_columns"] == deep == {"depths": 1, "deepest": 1 + ac.WIDE_COLUMNS}.get(name, 0)
    assert got["n_entries"] == sum(int(c["col_off"][-1] - c["col_off"][0]) for c in contigs)


@pytest.mark.parametrize("name", ["windows", "codes", "depths", "empty"])
def test_kernel_level_call_in_its_two_steps(built, lds_cap, name):
    """hs_group_alleles on device pointers: the plan covers every window and SNP of the call (SNPs in no window get no cells, windows without SNPs no
    groups); the cells of the second step, SNP by SNP, are the table's"""
    from hairsplitter_amd import api
    contigs, sr = ac.get(name, lds_cap)
    want = ac.rule_brute(contigs, sr)
    got = api.group_alleles(contigs, sr)
    in_table = got["snp_win"] >= 0
    assert int(in_table.sum()) == len(want["snp_pos"]) and np.array_equal(got["grp_pack"], want["group_ids"])
    assert np.array_equal(got["cells"].astype(ac.CELL), want["cells"]) and np.array_equal(got["n_calls"][in_table], want["snp_n_calls"])
    assert np.all(got["n_calls"][~in_table] == 0) and np.all(np.diff(got["cell_off"])[~in_table] == 0)
    has = got["win_snp_last"] > got["win_snp_first"]
    assert int(has.sum()) == len(want["win_start"]) and np.all(got["grp_n"][~has] == 0)
    assert np.array_equal(np.diff(got["grp_off"]), got["grp_n"])
    if name == "windows":
        assert (~in_table).sum() == 2 and (~has).sum() == 2


def test_the_call_refuses_what_it_cannot_describe(built):
    from hairsplitter_amd import api
    contigs, sr = ac.get("labels")
    bad = dict(sr, labels=sr["labels"][:-1], label_off=sr["label_off"] - np.array([0, 0, 1]))
    with pytest.raises(api.HsError):
        api.haplotype_alleles(contigs, bad)
    swapped = [dict(contigs[0], snp_pos=contigs[0]["snp_pos"][::-1].copy())]
    with pytest.raises(api.HsError):
        api.haplotype_alleles(swapped, sr)


def _job():
    """the `multi` job of the chain tests: three haplotypes, a contig too short for SNPs, one without reads, four haplotypes with clipped reads"""
    from hairsplitter_amd import synth
    return [synth.make_contig(12, 0, 9_000, 3, 0.01, 35, "ont"), synth.make_contig(12, 1, 700, 1, 0.0, 20, "ont", read_len_override=(100, 600)),
            synth.make_contig(12, 2, 5_000, 1, 0.0, 0, "ont"), synth.make_contig(12, 3, 20_011, 4, 0.012, 50, "ont", clip_prob=0.4)]


def test_separate_reads_route_drops_rare_snps_before_the_table(built):
    """api.separate_reads(alleles=True): SNPs below rarest_strain_abundance (separate_reads.cpp:167) are in neither the windows' runs nor the table"""
    from hairsplitter_amd import api, synth
    contigs = [synth.make_contig(7, 0, 12_000, 2, 0.01, 30, "ont")]
    flat = api.FlatBatch(contigs)
    b = api.CvBatch(flat)
    cv = b.run(0.33)
    b.close()
    er = min(float("%g" % np.float32(cv["error_rate"])), 0.15)
    seg = np.repeat(np.arange(len(cv["snp_pos"])), np.diff(cv["col_off"]))
    n_ref = np.bincount(seg, weights=cv["col_code"] == cv["snp_ref"][seg], minlength=len(cv["snp_pos"]))
    n_alt = np.bincount(seg, weights=cv["col_code"] == cv["snp_alt"][seg], minlength=len(cv["snp_pos"]))
    ratio = n_alt / np.maximum(n_ref + n_alt, 1)
    rsa = float(np.sort(ratio)[len(ratio) // 3]) + 1e-4
    out = api.separate_reads(cv, flat, er, rarest_strain_abundance=rsa, taps=True, alleles=True)
    kept = sum(len(c["snp_pos"]) for c in out["contigs"])
    assert 0 < kept < len(cv["snp_pos"])
    want = ac.rule_brute(out["contigs"], out)
    assert ac.differences(want, out["alleles"]) == []
    assert len(out["alleles"]["snp_pos"]) <= kept and len(out["alleles"]["cells"]) > 0 and (out["alleles"]["snp_n_calls"] >= 2).any()


def _group_columns(pg, rsa):
    """per-contig stage-4 inputs from the groups' stage-3 results of the last call (HS_PIPELINE_KEEP_COLUMNS), SNPs below rsa dropped"""
    import ctypes as C
    from hairsplitter_amd import api
    lib = api.load()
    lib.hs_pipeline_group_cv.restype = C.POINTER(api.CvResult)
    out = []
    for g in range(lib.hs_pipeline_groups(pg.handle)):
        r = lib.hs_pipeline_group_cv(pg.handle, C.c_int32(g)).contents
        S = int(r.snp_off[r.n_contigs]); E = int(r.col_off[S])
        a = lambda p, n, dt: np.ctypeslib.as_array(p, (max(n, 1),))[:n].astype(dt)
        snp_off, col_off = a(r.snp_off, r.n_contigs + 1, np.int64), a(r.col_off, S + 1, np.int64)
        pos, ref, alt = a(r.snp_pos, S, np.int32), a(r.snp_ref, S, np.uint8), a(r.snp_alt, S, np.uint8)
        n_ref, n_alt = a(r.snp_n_ref, S, np.int64), a(r.snp_n_alt, S, np.int64)
        idx, code = a(r.col_idx, E, np.int32), a(r.col_code, E, np.uint8)
        keep = n_alt.astype(np.float32) >= np.float32(rsa) * (n_ref + n_alt).astype(np.float32)
        for c in range(r.n_contigs):
            ss = [s for s in range(int(snp_off[c]), int(snp_off[c + 1])) if keep[s]]
            ents = [np.arange(col_off[s], col_off[s + 1]) for s in ss]
            ent = np.concatenate(ents).astype(np.int64) if ents else np.zeros(0, np.int64)
            out.append({"snp_pos": pos[ss], "snp_ref": ref[ss], "snp_alt": alt[ss], "col_idx": idx[ent], "col_code": code[ent],
                        "col_off": np.concatenate(([0], np.cumsum([len(e) for e in ents]))).astype(np.int64)})
    return out


def test_pipeline_option_gives_the_table_of_the_calls_own_labels(built):
    """HS_PIPELINE_ALLELES with two contig groups, two-call and fused form, dense and sparse labels, with and without HS_PIPELINE_KEEP_COLUMNS: one table,
    equal to hs_haplotype_alleles and to the numpy form on the call's labels and kept columns; labels and n_columns_downloaded as with the option off"""
    from hairsplitter_amd import api
    contigs = _job()
    pg = api.PipelineGroups(contigs, 2)
    try:
        cv0, sr0 = pg.run(0.33, 8)
        labels0 = sr0["labels"].copy()
        assert "alleles" not in sr0
        pg.alleles(True)
        tables = []
        for fused in (False, True):
            cv1, sr1 = pg.run_fused(0.33, 8) if fused else pg.run(0.33, 8)
            assert np.array_equal(sr1["labels"], labels0) and np.array_equal(sr1["win_start"], sr0["win_start"])
            assert cv1["n_columns_downloaded"] == cv0["n_columns_downloaded"] and cv1["n_snps"] == cv0["n_snps"]
            tables.append(sr1["alleles"])
        pg.keep_columns(True)
        cv2, sr2 = pg.run_fused(0.33, 8)
        tables.append(sr2["alleles"])
        assert np.array_equal(sr2["labels"], labels0)
        cols = _group_columns(pg, 0.01)
        assert len(cols) == len(contigs)
        n_reads = np.diff(pg.flat.contig_rec_off)
        for c, ctg in enumerate(cols):
            ctg.update(length=int(pg.flat.contig_off[c + 1] - pg.flat.contig_off[c]), read_start=np.zeros(n_reads[c], np.int32), read_end=np.zeros(n_reads[c], np.int32))
        sr_in = {k: sr2[k] for k in ("win_off", "win_start", "win_end", "label_off")}
        sr_in["labels"] = labels0
        tables.append(api.haplotype_alleles(cols, sr_in))
        want = ac.rule_numpy(cols, sr_in)
        pg.sparse_labels(True)
        for fused in (False, True):
            cv3, sr3 = pg.run_fused(0.33, 8) if fused else pg.run(0.33, 8)
            assert sr3["labels"] is None
            tables.append(sr3["alleles"])
        for k, t in enumerate(tables):
            assert ac.differences(want, t) == [], k
        assert len(want["cells"]) > 100 and set(want["win_contig"].tolist()) == {0, 3} and (want["snp_n_calls"] >= 2).any()
        pg.alleles(False)
        assert "alleles" not in pg.run_fused(0.33, 8)[1]
    finally:
        pg.close()


_VIA_HOST = """
import sys, zlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_alleles as t
from hairsplitter_amd import api
pg = api.PipelineGroups(t._job(), 2)
pg.alleles(True)
a = pg.run_fused(0.33, 8)[1]["alleles"]
print("TABLE", len(a["cells"]), zlib.crc32(b"".join(a[k].tobytes() for k in t.ac.TABLE_KEYS)))
pg.close()
"""


def test_pipeline_table_is_the_same_with_the_columns_handed_over_through_the_host(built):
    """HS_COLUMNS_VIA_HOST=1 (read once per process: a child): stage 4 uploads the columns itself, the groups' shares come out the same"""
    import zlib
    from hairsplitter_amd import api
    pg = api.PipelineGroups(_job(), 2)
    try:
        pg.alleles(True)
        a = pg.run_fused(0.33, 8)[1]["alleles"]
    finally:
        pg.close()
    want = "TABLE %d %d" % (len(a["cells"]), zlib.crc32(b"".join(a[k].tobytes() for k in ac.TABLE_KEYS)))
    r = subprocess.run([sys.executable, "-c", _VIA_HOST % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, HS_COLUMNS_VIA_HOST="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and want in r.stdout.decode().splitlines(), r.stdout.decode()[-2000:]


def test_executable_writes_the_table_of_its_own_run(built):
    """HS_ALLELES=1: the .gro is byte-identical with and without it (and the precomputed .gro is not adopted), <outfile>.alleles.tsv is the text of the
    table the API gives on the .gro's labels and the .col's columns; without the variable no such file"""
    from hairsplitter_amd import api, canon
    with tempfile.TemporaryDirectory() as td:
        meta = gu.unpack("multi", td)
        env = dict(os.environ, HS_NO_DETACH="1")
        col = os.path.join(td, "variants.col")
        er = meta["error_rate_arg"]

        def stage4(out, env):
            r = subprocess.run([built["sr"], col, "1", er, os.path.join(td, "no_ploidy"), "0", "0.01", "0", os.path.join(td, out), "0"],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
            assert r.returncode == 0, r.stdout.decode()[-2000:]
            return open(os.path.join(td, out), "rb").read()

        plain = stage4("a.gro", env)
        with_table = stage4("b.gro", dict(env, HS_ALLELES="1"))
        assert plain == with_table and len(plain) > 0
        assert not os.path.exists(os.path.join(td, "a.gro.alleles.tsv"))
        text = open(os.path.join(td, "b.gro.alleles.tsv")).read()
        # the same table in process: the .col's columns (SNPs under 0.01 dropped, as the executable's reader drops them) and the .gro's labels
        names, contigs, sr = _col_and_gro(col, os.path.join(td, "b.gro"), 0.01)
        assert len(canon.split_blocks(col)) == len(names)
        table = api.haplotype_alleles(contigs, sr)
        assert ac.differences(ac.rule_numpy(contigs, sr), table) == []
        assert text == api.alleles_text(table, names) and text.count("WINDOW\t") == len(table["win_start"]) > 0


def _col_and_gro(col_path, gro_path, rsa):
    """(contig names, per-contig stage-4 inputs, windows + dense labels) from a .col and the .gro made from it"""
    names, contigs, cur = [], [], None
    for line in open(col_path):
        f = line.rstrip("\n").split("\t")
        if f[0] == "CONTIG":
            cur = {"length": int(f[2]), "reads": [], "snp_pos": [], "snp_ref": [], "snp_alt": [], "idx": [], "code": []}
            names.append(f[1]); contigs.append(cur)
        elif f[0] == "READ":
            cur["reads"].append(f[1])
        elif f[0] == "SNPS":
            ref, alt = int(f[2]), int(f[3])
            idx = [int(x) for x in f[4].split(",") if x != ""]
            code = [int(x) for x in f[5].split(",") if x != ""] if len(f) > 5 else []
            assert len(idx) == len(code)
            n_ref, n_alt = sum(1 for k in code if k == ref), sum(1 for k in code if k == alt and k != ref)
            if not (np.float32(n_alt) >= np.float32(rsa) * np.float32(n_ref + n_alt)):
                continue
            cur["snp_pos"].append(int(f[1])); cur["snp_ref"].append(ref); cur["snp_alt"].append(alt); cur["idx"].append(idx); cur["code"].append(code)
    out = []
    for c in contigs:
        n = len(c["reads"])
        out.append({"length": c["length"], "read_start": np.zeros(n, np.int32), "read_end": np.zeros(n, np.int32), "snp_pos": np.array(c["snp_pos"], np.int32),
                    "snp_ref": np.array(c["snp_ref"], np.uint8), "snp_alt": np.array(c["snp_alt"], np.uint8),
                    "col_off": np.concatenate(([0], np.cumsum([len(i) for i in c["idx"]]))).astype(np.int64),
                    "col_idx": np.array([x for i in c["idx"] for x in i], np.int32), "col_code": np.array([x for k in c["code"] for x in k], np.uint8)})
    # the .gro: per contig its windows, one label per READ line of the .col
    win = {name: [] for name in names}
    cur = None
    for line in open(gro_path):
        f = line.rstrip("\n").split("\t")
        if f[0] == "CONTIG":
            cur = f[1]
        elif f[0] == "GROUP":
            win[cur].append((int(f[1]), int(f[2]), [int(x) for x in f[3].split(",") if x != ""], [int(x) for x in f[4].split(",") if x != ""]))
    win_off, ws, we, lo, lab = [0], [], [], [0], []
    for name, c in zip(names, out):
        n = len(c["read_start"])
        for a, b, ids, labels in win[name]:
            row = np.full(n, -2, np.int32)
            row[ids] = labels
            ws.append(a); we.append(b); lab.append(row); lo.append(lo[-1] + n)
        win_off.append(len(ws))
    sr = {"win_off": np.array(win_off, np.int64), "win_start": np.array(ws, np.int32), "win_end": np.array(we, np.int32), "label_off": np.array(lo, np.int64),
          "labels": np.concatenate(lab) if lab else np.zeros(0, np.int32)}
    return names, out, sr
