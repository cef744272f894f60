"""The host side of the allele table without a device (hs_alleles_host.h / .cpp through tests/harness/alleles_selftest.cpp): the cell rule the kernel ends
in, the assembly of the table, the merge of two contig groups' tables and the text writer, on every case of tests/allele_cases.py, against rule_brute and
the Python writer hairsplitter_amd.api.alleles_text."""
import os
import subprocess

import pytest

import allele_cases as ac


def _stdin_of(contigs, sr, split):
    out = ["%d %d" % (len(contigs), split)]
    for c in contigs:
        out.append("%d %d" % (len(c["read_start"]), len(c["snp_pos"])))
        for s in range(len(c["snp_pos"])):
            a, b = int(c["col_off"][s]), int(c["col_off"][s + 1])
            out.append("%d %d %d %d" % (c["snp_pos"][s], c["snp_ref"][s], c["snp_alt"][s], b - a))
            out.append(" ".join("%d %d" % (i, k) for i, k in zip(c["col_idx"][a:b].tolist(), c["col_code"][a:b].tolist())))
    out.append("%d" % len(sr["win_start"]))
    out.append(" ".join(str(int(x)) for x in sr["win_off"]))
    for w in range(len(sr["win_start"])):
        out.append("%d %d" % (sr["win_start"][w], sr["win_end"][w]))
        out.append(" ".join(str(int(x)) for x in sr["labels"][int(sr["label_off"][w]):int(sr["label_off"][w + 1])]))
    return ("\n".join(out) + "\n").encode()


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_host_table_and_text_match_the_rule(built, name):
    from hairsplitter_amd import api
    exe = os.path.join(os.path.dirname(built["harness"]), "alleles_selftest")
    contigs, sr = ac.get(name, 300)
    want = api.alleles_text(ac.rule_brute(contigs, sr), ["c%d" % c for c in range(len(contigs))])
    for split in sorted({0, len(contigs) // 2, len(contigs)}):
        r = subprocess.run([exe], input=_stdin_of(contigs, sr, split), stdout=subprocess.PIPE, check=True)
        assert r.stdout.decode() == want, (name, split)
    if name == "codes":
        # 47 = '!' + 5 * 2 + 4 + 25 * 0: G before, a gap, A behind (call_variants.cpp:25-31, :238)
        assert "SNP\t50\tG\t-\t1\t0:10:5:5:.\t1:9:0:9:G-A\n" in want and api.allele_context(40) == "CGA" and api.allele_context(0) == "."
