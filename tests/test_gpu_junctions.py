"""The GPU junction finder (csrc/junctions.hip behind lcb_junctions_build, sibeliaz_amd.build_junctions and `lcb-mkgraph --gpu`):
the file it writes equals, byte for byte, what the CPU tool lcb-mkgraph writes in the same test - and the committed golden graphs
and the brute-force finder of tests/test_mkgraph.py where stated. The options (table size, tile size) never change the bytes."""
import gzip
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from tests import edge_inputs as E
from tests.conftest import Case
from tests.test_mkgraph import brute_force_junctions, read_fasta, read_junction_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sibeliaz_amd", "bin")
MKGRAPH = os.path.join(BIN, "lcb-mkgraph")
COMP = str.maketrans("ACGT", "TGCA")


def cpu_graph(fasta, k, out):
    subprocess.check_call([MKGRAPH, "-k", str(k), "-o", out] + list(fasta), stderr=subprocess.DEVNULL)
    return open(out, "rb").read()


def gpu_graph(fasta, k, out, **opts):
    stats = sibeliaz_amd.build_junctions(list(fasta), k, out, **opts)
    assert not os.path.exists(out + ".part")
    return open(out, "rb").read(), stats


def check_stats(stats, data, n_records):
    assert stats["records"] == n_records
    assert len(data) == 12 * (stats["occurrences"] + n_records)
    assert stats["table_slots"] & (stats["table_slots"] - 1) == 0


@pytest.mark.parametrize("k", [None, 11])
def test_goldens(built, case, k, tmp_path):
    k = k or case.k
    want = cpu_graph([case.fasta], k, str(tmp_path / "cpu.bin"))
    got, stats = gpu_graph([case.fasta], k, str(tmp_path / "gpu.bin"))
    assert got == want
    check_stats(stats, got, len(read_fasta(case.fasta)))
    if k == case.k:
        with gzip.open(os.path.join(case.dir, "graph.bin.gz"), "rb") as f:
            assert f.read() == got


@pytest.mark.parametrize("name", E.NAMES)
def test_edge_inputs(built, name, tmp_path):
    c = E.build(name, str(tmp_path))
    got, _ = gpu_graph(c["fasta"], c["k"], str(tmp_path / "gpu.bin"))
    assert got == open(c["graph"], "rb").read()


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _small_inputs():
    rng = random.Random(20)
    a, b = _rand(rng, 400), _rand(rng, 300)
    out = {}
    # records without a window (shorter than k, empty, all N) between two normal ones: each still gets its separator
    out["no_window_records"] = (15, ">a\n%s\n>short\nACGTACG\n>empty\n>enn\n%s\n>b\n%s\n" % (a, "N" * 40, b + a[50:150]))
    out["exactly_k"] = (15, ">a\n%s\n>k\n%s\n>b\n%s\n" % (a, a[100:115], b))
    # every window in one slot, on both strands: the atomics under full contention
    out["homopolymer"] = (15, ">a\n%s\n>t\n%s\n" % ("A" * 5000, "T" * 5000))
    out["tandem"] = (15, ">r\n%s\n" % ("ACGG" * 750))
    out["k3_random"] = (3, ">r\n%s\n" % _rand(rng, 2000))          # at most 32 distinct keys: nearly every lane collides
    s = _rand(rng, 3000)
    t = "".join((rng.choice("ACGT") if rng.random() < 0.02 else c) for c in s)
    out["k31_strains"] = (31, ">s\n%s\n>t\n%s\n" % (s, t))          # 62-bit keys, the k-mer + 1 encoding
    return out


SMALL = _small_inputs()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_inputs_against_brute_force(built, name, tmp_path):
    k, text = SMALL[name]
    fa = str(tmp_path / "in.fa")
    with open(fa, "w") as f:
        f.write(text)
    want = cpu_graph([fa], k, str(tmp_path / "cpu.bin"))
    got, stats = gpu_graph([fa], k, str(tmp_path / "gpu.bin"))
    assert got == want
    recs = read_fasta(fa)
    assert read_junction_file(str(tmp_path / "gpu.bin")) == brute_force_junctions(recs, k)
    check_stats(stats, got, len(recs))
    assert stats["windows"] == sum(max(0, len(s) - k + 1) for _, s in recs)


def test_table_regrowth(built, tmp_path):
    rng = random.Random(3)
    fa = str(tmp_path / "rand.fa")
    with open(fa, "w") as f:
        f.write(">r\n%s\n" % _rand(rng, 200000))
    want = cpu_graph([fa], 25, str(tmp_path / "cpu.bin"))
    got, stats = gpu_graph([fa], 25, str(tmp_path / "gpu.bin"), table_log2=10)
    assert got == want
    assert stats["table_rebuilds"] >= 1
    slots = stats["table_slots"]
    assert slots & (slots - 1) == 0 and slots >= stats["windows"] / 0.9


@pytest.mark.parametrize("name,tile", [("nruns_abund", 64), ("nruns_abund", 4096), ("collinear6", 1000)])
def test_tiling(built, case_dir, name, tile, tmp_path):
    case = Case(name, case_dir)
    base, _ = gpu_graph([case.fasta], case.k, str(tmp_path / "default.bin"))
    got, stats = gpu_graph([case.fasta], case.k, str(tmp_path / "tiled.bin"), tile_windows=tile)
    assert stats["tiles"] > 1
    assert got == base
    assert got == cpu_graph([case.fasta], case.k, str(tmp_path / "cpu.bin"))


def test_determinism(built, case_dir, tmp_path):
    case = Case("nruns_abund", case_dir)
    a, _ = gpu_graph([case.fasta], case.k, str(tmp_path / "a.bin"))
    b, _ = gpu_graph([case.fasta], case.k, str(tmp_path / "b.bin"))
    c, _ = gpu_graph([case.fasta], case.k, str(tmp_path / "c.bin"), table_log2=18, tile_windows=777)
    assert a == b == c


def test_more_than_one_of_everything(built, tmp_path):
    """Several Mbp: more than 2^20 windows per record, a default table above the minimum, many workgroups, several default tiles."""
    fa = str(tmp_path / "synth.fa")
    subprocess.check_call([os.path.join(BIN, "lcb-synth"), "-o", fa] + "--strains 8 --segments 400 --seg-min 1000 --seg-max 4000 --sub 0.03 --indel 0.004 --invert 0.1 "
                          "--repeat-families 4 --repeat-copies 6 --repeat-len 500 --nrun 0.01 --seed 7".split())
    want = hashlib.sha256(cpu_graph([fa], 25, str(tmp_path / "cpu.bin"))).hexdigest()
    got, stats = gpu_graph([fa], 25, str(tmp_path / "gpu.bin"))
    assert hashlib.sha256(got).hexdigest() == want
    assert stats["windows"] > (1 << 21) and stats["table_slots"] > (1 << 20)


def test_tool_gpu_flag(built, case_dir, tmp_path):
    case = Case("twogenomes", case_dir)
    cpu = subprocess.run([MKGRAPH, "-k", "15", "-o", str(tmp_path / "cpu.bin"), case.fasta], capture_output=True, text=True, check=True)
    env = {k: v for k, v in os.environ.items() if k != "LCB_LIB"}
    gpu = subprocess.run([MKGRAPH, "--gpu", "0", "-k", "15", "-o", str(tmp_path / "gpu.bin"), case.fasta], capture_output=True, text=True, env=env)
    assert gpu.returncode == 0, gpu.stderr
    with gzip.open(os.path.join(case.dir, "graph.bin.gz"), "rb") as f:
        assert f.read() == open(str(tmp_path / "gpu.bin"), "rb").read()
    summary = r"lcb-mkgraph: (\d+) records, (\d+) junction occurrences, (\d+) junction k-mers"
    assert re.search(summary, gpu.stderr).groups() == re.search(summary, cpu.stderr).groups()


def test_loader_accepts_the_gpu_file(built, case_dir, tmp_path):
    case = Case("inv_k25", case_dir)
    out = str(tmp_path / "gpu.bin")
    gpu_graph([case.fasta], case.k, out)
    ours = sibeliaz_amd.JunctionStorage(out, [case.fasta], case.k, 2, case.a)
    gold = sibeliaz_amd.JunctionStorage(case.graph, [case.fasta], case.k, 2, case.a)
    assert np.array_equal(ours.pos_id(), gold.pos_id())
    assert np.array_equal(ours.pos_pos(), gold.pos_pos())
