"""The polisher's inputs of the reference's stage 5 without a GPU: the per-base restatement (polish_restatement.py) alone
reproduces what the compiled reference handed to its polisher (tests/golden/polish_inputs, tools/record_polish_goldens.py), so
the two oracles of test_gpu_polish_inputs.py agree and the recordings are consistent with the inputs they name; the header
declares the entry points; the tool refuses to run without arguments."""
import os
import re
import subprocess
import tempfile

import pytest

import polish_goldens as pg
import polish_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_linked_with_polish_everything_is_recorded():
    assert "linked_p1" in [r[0] for r in pg.recorded_runs()]
    assert len(pg.load("linked_p1")["bundles"]) == 9


@pytest.mark.parametrize("run,source,polish", pg.recorded_runs(), ids=[r[0] for r in pg.recorded_runs()])
def test_restatement_reproduces_the_reference_bytes(run, source, polish):
    rec = pg.load(run)
    with tempfile.TemporaryDirectory() as td:
        gfa, reads, sam, gro = pg.prepare(source, td)
        assert pg.inputs_digest((gfa, reads, sam, gro)) == rec["inputs_sha1"], "the inputs are not the ones the recording was made from"
        bundles, _, _ = pr.job_bundles(gfa, reads, sam, gro, bool(polish))
    assert rec["polish_everything"] == polish
    assert pr.restated_keys(bundles) == rec["keys"]


def test_walk_rules():
    """the rules of create_new_contigs.cpp:392-447 the issue names, on the restatement itself"""
    # an insertion exactly at leftToPolish is inside the piece; S and H both advance the read cursor before the start
    assert pr.walk(pr.convert_cigar("3H2S5M2I5M"), 0, 5, 8)[:2] == (10, 15)
    # '=' 'X' 'N' advance nothing: the end condition is never met, the piece runs to the end of the walk
    assert pr.walk(pr.convert_cigar("4=4X"), 0, 0, 3) == (0, 0, 0, 8)
    # a deletion over the whole range: the end comes at the first char at which the cursor == rightToPolish
    assert pr.cut_read("ACGTACGTAC", True, "2M30D8M", 0, 10, 20) is not None
    assert pr.cut_read("ACGT", True, "4M", 100, 10, 20)["bases"] == "ACGT"      # begins beyond the range: taken whole
    assert pr.cut_read("ACGT", True, "4S", 0, 0, 20) is None                       # never a non-clip char: dropped
    assert pr.convert_cigar2("MMMDDMM") == "3M2D2M"


def test_header_declares_the_polish_symbols():
    from hairsplitter_amd import api
    hdr = open(os.path.join(ROOT, "include", "hairsplitter_hip.h")).read()
    for sym in ("hs_polish_inputs", "hs_polish_inputs_from_files", "hs_polish_result_destroy", "hs_polish_inputs_main"):
        assert re.search(r"\b%s\(" % sym, hdr), sym
        assert sym in api.SYMBOLS
    assert "typedef struct hs_polish_result" in hdr


def test_tool_usage(built):
    r = subprocess.run([built["polish_inputs"]], stdout=subprocess.PIPE)
    assert r.returncode == 1 and b"Usage: hs_polish_inputs" in r.stdout
    assert subprocess.run([built["polish_inputs"], "--help"], stdout=subprocess.DEVNULL).returncode == 0
