"""The host side of the recruit table without a device (hs_recruit_host.h / .cpp through tests/harness/recruit_selftest.cpp): the rule functions the kernels
end in, the assembly of the table, the merge of two contig groups' tables, hs_recruit_apply and the text writer, on every case of tests/recruit_cases.py, against
recruit_brute and the Python statement of the text."""
import os
import subprocess

import pytest

import recruit_cases as rc
from test_cpu_recruit_cases import RUNS


def _exe(built):
    return os.path.join(os.path.dirname(built["harness"]), "recruit_selftest")


@pytest.mark.parametrize("name,i", RUNS)
def test_host_table_text_and_labels_match_the_rule(built, tmp_path, name, i):
    ctgs, sr, prms = rc.get(name)
    t = rc.recruit_brute(ctgs, sr, prms[i])
    want = rc.text(t, ["c%d" % c for c in range(len(ctgs))])
    want += "LABELS\n" + "".join("%d " % v for v in rc.apply_numpy(t, sr)) + "\n"
    want += "ASSIGNED %d OF %d IN %d WINDOWS OF %d\n" % (int((t["rows"]["assigned"] != 0).sum()), len(t["rows"]), len(t["win_start"]), len(sr["win_start"]))
    for split in sorted({0, len(ctgs) // 2, len(ctgs)}):
        path = tmp_path / ("call%d.json" % split)
        path.write_text(rc.host_input(ctgs, sr, prms[i], split))
        r = subprocess.run([_exe(built), str(path)], stdout=subprocess.PIPE, check=True)
        assert r.stdout.decode() == want, (name, i, split)
    if (name, i) == ("rule", 0):
        assert "READ\t15\t-2\t0\t3\t1\t5\t1\t3\t4\t1\n" in want and want.startswith("WINDOW\tc0\t0\t999\n")


@pytest.mark.parametrize("bad", rc.REFUSED)
def test_refused_thresholds(built, tmp_path, bad):
    ctgs, sr, _ = rc.get("rule")
    path = tmp_path / "call.json"
    path.write_text(rc.host_input(ctgs, sr, rc.params(**bad), 0))
    assert subprocess.run([_exe(built), str(path)], stdout=subprocess.PIPE).returncode == 4
