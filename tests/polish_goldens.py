"""The recorded polisher inputs of the reference (tests/golden/polish_inputs/<run>.json.gz, written by
tools/record_polish_goldens.py): which runs there are, how their input files are made, and how a recording is read."""
import gzip
import hashlib
import json
import os
import random
import shutil

import golden_util as gu

DIR = os.path.join(gu.GOLD, "polish_inputs")
CASES = ["linked", "clips", "edge_ops", "multi", "dip10k_fastq"]
RANDOM = ("linked", "rough", 2)      # the three .gro files of test_cpu_gaf.RANDOM_PARTITIONS[1]


def run_names():
    """[(run, source, polish_everything)]: source = a golden case or ("random", rep)"""
    out = []
    for p in (0, 1):
        for c in CASES:
            out.append(("%s_p%d" % (c, p), c, p))
        for rep in range(3):
            out.append(("%s_%s_%d_%d_p%d" % (RANDOM + (rep, p)), ("random", rep), p))
    return out


def prepare(source, td):
    """unpacks the inputs of a run into td; returns (gfa, reads, sam, gro)"""
    case = RANDOM[0] if isinstance(source, tuple) else source
    meta = gu.unpack(case, td)
    gro = os.path.join(td, "reads_haplo.gro")
    if isinstance(source, tuple):
        from test_cpu_gaf import _random_gro
        rng = random.Random(RANDOM[2])
        for rep in range(source[1] + 1):      # the generator's state runs through the repetitions
            gro = _random_gro(td, rng, RANDOM[1])
        shutil.copy(gro, os.path.join(td, "random_%d.gro" % source[1]))
        gro = os.path.join(td, "random_%d.gro" % source[1])
    return os.path.join(td, "assembly.gfa"), gu.reads_path(td, meta), os.path.join(td, "aln.sam"), gro


def inputs_digest(paths):
    h = hashlib.sha1()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def path_of(run):
    return os.path.join(DIR, run + ".json.gz")


def recorded_runs():
    return [r for r in run_names() if os.path.exists(path_of(r[0]))]


def load(run):
    with gzip.open(path_of(run), "rt") as f:
        d = json.load(f)
    d["keys"] = sorted((b[0], b[1], tuple(tuple(x) for x in b[2])) for b in d["bundles"])
    return d
