#!/usr/bin/env python3
"""Records what the reference hands to its polisher (tests/golden/polish_inputs/<run>.json.gz): its compiled
HS_create_new_contigs (oracle/_ref, `make -C oracle ref`) runs on the inputs of every run of tests/polish_goldens.py with three
stand-in executables of ours in place of the external tools:
  minimap2  on the plain "-a -t 1 -x map-pb" call of consensus_reads it copies its last two arguments (unpolished_<id>.fasta,
            reads_<id>.fasta) into a capture directory and exits 0; it exits 0 on the --secondary=no calls and 1 on ava-ont;
  samtools  exits 0;  racon exits 1.
Only recorded data are stored: per bundle the length and SHA-1 of toPolish, per read its index, length and CRC-32, and a digest
of the input files. A run the reference does not finish with exit status 0 is not stored.

    python tools/record_polish_goldens.py [run ...]"""
import gzip
import json
import os
import stat
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import polish_goldens as pg          # noqa: E402
import polish_restatement as pr      # noqa: E402

MINIMAP2 = """#!/bin/sh
case " $* " in
  *" --secondary=no "*) exit 0 ;;
  *ava-ont*) exit 1 ;;
esac
for a in "$@"; do prev="$last"; last="$a"; done
d=$(mktemp -d "$HS_POLISH_CAPTURE/b.XXXXXXXX") || exit 1
cp "$prev" "$d/unpolished.fasta" && cp "$last" "$d/reads.fasta"
exit 0
"""


def _script(path, text):
    with open(path, "w") as f:
        f.write(text)
    os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)


def record(ref_cnc, source, polish):
    with tempfile.TemporaryDirectory() as td:
        gfa, reads, sam, gro = pg.prepare(source, td)
        tools, cap, tmp = (os.path.join(td, d) for d in ("standins", "capture", "cnc_tmp"))
        for d in (tools, cap, tmp):
            os.makedirs(d)
        _script(os.path.join(tools, "minimap2"), MINIMAP2)
        _script(os.path.join(tools, "samtools"), "#!/bin/sh\nexit 0\n")
        _script(os.path.join(tools, "racon"), "#!/bin/sh\nexit 1\n")
        env = dict(os.environ, HS_POLISH_CAPTURE=cap, PATH=tools + os.pathsep + os.environ.get("PATH", ""))
        r = subprocess.run([ref_cnc, gfa, reads, "0.05", gro, sam, tmp + "/", "1", "ont", os.path.join(tmp, "o.gfa"), os.path.join(tmp, "o.gaf"), "racon",
                            str(polish), "0", os.path.join(tools, "minimap2"), os.path.join(tools, "racon"), "/nonexistent/medaka",
                            os.path.join(tools, "samtools"), "/nonexistent/python", "0"], cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode != 0:
            return None, r.stdout.decode(errors="replace")[-1500:]
        bundles = []
        for d in sorted(os.listdir(cap)):
            un = open(os.path.join(cap, d, "unpolished.fasta"), "rb").read().split(b"\n")
            rd = open(os.path.join(cap, d, "reads.fasta"), "rb").read().split(b"\n")
            assert un[0] == b">seq"
            pieces = [(int(rd[i][5:]), rd[i + 1]) for i in range(0, len(rd) - 1, 2)]
            assert all(rd[i].startswith(b">read") for i in range(0, len(rd) - 1, 2))
            k = pr.bundle_key(un[1], pieces)
            bundles.append([k[0], k[1], [list(x) for x in k[2]]])
        bundles.sort()
        return {"polish_everything": polish, "inputs_sha1": pg.inputs_digest((gfa, reads, sam, gro)), "bundles": bundles}, ""


def main():
    import __graft_entry__ as ge
    ref_cnc = ge.paths()["ref_cnc"]
    if not os.path.exists(ref_cnc):
        sys.exit("oracle/_ref/HS_create_new_contigs is missing: make -C oracle ref (needs the reference's sources)")
    os.makedirs(pg.DIR, exist_ok=True)
    for run, source, polish in pg.run_names():
        if len(sys.argv) > 1 and run not in sys.argv[1:]:
            continue
        rec, err = record(ref_cnc, source, polish)
        if rec is None:
            print("%s: NOT recorded, the reference failed: %s" % (run, err.strip().splitlines()[-1] if err.strip() else "no output"))
            continue
        with gzip.GzipFile(pg.path_of(run), "wb", mtime=0) as f:
            f.write(json.dumps(rec, separators=(",", ":")).encode())
        print("%s: %d bundles, %d reads" % (run, len(rec["bundles"]), sum(len(b[2]) for b in rec["bundles"])))


if __name__ == "__main__":
    main()
