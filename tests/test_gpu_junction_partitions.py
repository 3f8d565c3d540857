"""The partitioned GPU junction build (lcb_junctions_build_ex behind sibeliaz_amd.build_junctions(partitions=, mem_budget=) and
`lcb-mkgraph --gpu --partitions`): the k-mer table is built in P passes over parts of the canonical k-mer space, and the file is, byte
for byte, what the CPU tool lcb-mkgraph writes - for every P, every table capacity and every tile size."""
import gzip
import hashlib
import os
import random
import re
import subprocess

import pytest

import sibeliaz_amd
from tests.conftest import Case
from tests.test_junction_partitions_emu import INPUTS as SMALL
from tests.test_mkgraph import read_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sibeliaz_amd", "bin")
MKGRAPH = os.path.join(BIN, "lcb-mkgraph")
_cpu = {}


def cpu_graph(name, fasta, k, tmp_path):
    """The CPU tool's file for an input, computed once and shared between the cases of that input."""
    if name not in _cpu:
        out = str(tmp_path / "cpu.bin")
        subprocess.check_call([MKGRAPH, "-k", str(k), "-o", out, fasta], stderr=subprocess.DEVNULL)
        _cpu[name] = open(out, "rb").read()
    return _cpu[name]


def gpu_graph(fasta, k, out, **opts):
    stats = sibeliaz_amd.build_junctions([fasta], k, out, **opts)
    assert not os.path.exists(out + ".part")
    return open(out, "rb").read(), stats


def check_stats(stats, data, n_records, partitions):
    assert stats["partitions"] == partitions and stats["passes"] >= partitions
    assert stats["records"] == n_records and len(data) == 12 * (stats["occurrences"] + n_records)
    assert stats["junction_windows"] == stats["occurrences"]
    for f in ("table_slots", "junction_table_slots"):
        assert stats[f] > 0 and stats[f] & (stats[f] - 1) == 0
    assert stats["junction_table_slots"] * 9 >= stats["junction_kmers"] * 10
    assert stats["peak_device_bytes"] >= 12 * stats["table_slots"]


@pytest.mark.parametrize("partitions", [2, 3, 8])
@pytest.mark.parametrize("name", ["twogenomes", "nruns_abund", "collinear6", "inv_k25"])
def test_goldens(built, case_dir, name, partitions, tmp_path):
    case = Case(name, case_dir)
    got, stats = gpu_graph(case.fasta, case.k, str(tmp_path / "gpu.bin"), partitions=partitions)
    assert got == cpu_graph(name, case.fasta, case.k, tmp_path)
    with gzip.open(os.path.join(case.dir, "graph.bin.gz"), "rb") as f:
        assert f.read() == got
    check_stats(stats, got, len(read_fasta(case.fasta)), partitions)


@pytest.mark.parametrize("partitions", [2, 7, 64])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_inputs(built, name, partitions, tmp_path):
    k, table_log2, tile, text = SMALL[name]
    fa = str(tmp_path / "in.fa")
    with open(fa, "w") as f:
        f.write(text)
    got, stats = gpu_graph(fa, k, str(tmp_path / "gpu.bin"), partitions=partitions, table_log2=table_log2, tile_windows=tile)
    assert got == cpu_graph("small_" + name, fa, k, tmp_path)
    check_stats(stats, got, len(read_fasta(fa)), partitions)


@pytest.fixture(scope="module")
def random_200k(tmp_path_factory):
    d = tmp_path_factory.mktemp("rand")
    rng = random.Random(3)
    fa = str(d / "rand.fa")
    with open(fa, "w") as f:
        f.write(">r\n%s\n" % "".join(rng.choice("ACGT") for _ in range(200000)))
    return fa, d


def test_regrowth_inside_every_partition(built, random_200k):
    fa, d = random_200k
    got, stats = gpu_graph(fa, 25, str(d / "gpu.bin"), partitions=4, table_log2=10)
    assert got == cpu_graph("random_200k", fa, 25, d)
    assert stats["table_rebuilds"] >= 4
    # 200 000 random 25-mers are all distinct, the fullest of 4 partitions holds at least a quarter of them, at a load of at most 0.9
    assert stats["table_slots"] * 0.9 >= stats["windows"] / 4
    check_stats(stats, got, 1, 4)


def test_determinism_with_small_tiles(built, random_200k):
    fa, d = random_200k
    a, sa = gpu_graph(fa, 25, str(d / "a.bin"), partitions=4, table_log2=10, tile_windows=777)
    b, _ = gpu_graph(fa, 25, str(d / "b.bin"), partitions=4, table_log2=10, tile_windows=777)
    assert sa["tiles"] > 200
    assert a == b == cpu_graph("random_200k", fa, 25, d)


@pytest.fixture(scope="module")
def synth8(built, tmp_path_factory):
    """The 8-strain input of tests/test_gpu_junctions.py::test_more_than_one_of_everything, its sizes and the CPU tool's sha256."""
    d = tmp_path_factory.mktemp("synth")
    fa = str(d / "synth.fa")
    subprocess.check_call([os.path.join(BIN, "lcb-synth"), "-o", fa] + "--strains 8 --segments 400 --seg-min 1000 --seg-max 4000 --sub 0.03 --indel 0.004 --invert 0.1 "
                          "--repeat-families 4 --repeat-copies 6 --repeat-len 500 --nrun 0.01 --seed 7".split())
    lens = [len(s) for _, s in read_fasta(fa)]
    windows, seq_bytes = sum(max(0, n - 25 + 1) for n in lens), sum(lens) + len(lens) + 1
    assert windows > (1 << 21)
    return fa, d, windows, seq_bytes, hashlib.sha256(cpu_graph("synth8", fa, 25, d)).hexdigest()


def test_automatic_choice_under_a_budget(built, synth8):
    fa, d, windows, seq_bytes, want = synth8
    one, need_one = sibeliaz_amd.plan_junctions(windows, seq_bytes, 0, partitions=1)
    budget = int(0.6 * need_one)
    planned, need = sibeliaz_amd.plan_junctions(windows, seq_bytes, budget)
    got, stats = gpu_graph(fa, 25, str(d / "gpu.bin"), mem_budget=budget, tile_windows=65536)
    print("need at P = 1: %d, budget %d, planned P = %d (need %d); stats %r" % (need_one, budget, planned, need, stats))
    assert one == 1 and stats["windows"] == windows
    assert stats["partitions"] == planned and planned > 1
    assert stats["peak_device_bytes"] <= budget
    assert hashlib.sha256(got).hexdigest() == want


def test_a_budget_below_the_sequence_fails_and_leaves_no_file(built, synth8):
    fa, d, windows, seq_bytes, _ = synth8
    out = str(d / "none.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match=str(seq_bytes // 2)):
        sibeliaz_amd.build_junctions([fa], 25, out, mem_budget=seq_bytes // 2, tile_windows=65536)
    assert not os.path.exists(out) and not os.path.exists(out + ".part")


def test_tool_partitions_flag(built, case_dir, tmp_path):
    case = Case("twogenomes", case_dir)
    cpu = subprocess.run([MKGRAPH, "-k", "15", "-o", str(tmp_path / "cpu.bin"), case.fasta], capture_output=True, text=True, check=True)
    env = {k: v for k, v in os.environ.items() if k != "LCB_LIB"}
    env["LCB_MKGRAPH_VERBOSE"] = "1"
    with gzip.open(os.path.join(case.dir, "graph.bin.gz"), "rb") as f:
        gold = f.read()
    summary = r"lcb-mkgraph: (\d+) records, (\d+) junction occurrences, (\d+) junction k-mers"
    for flag, parts in (("3", "3"), ("auto", "1")):
        out = str(tmp_path / ("gpu_%s.bin" % flag))
        gpu = subprocess.run([MKGRAPH, "--gpu", "0", "--partitions", flag, "-k", "15", "-o", out, case.fasta], capture_output=True, text=True, env=env)
        assert gpu.returncode == 0, gpu.stderr
        assert open(out, "rb").read() == gold
        assert re.search(summary, gpu.stderr).groups() == re.search(summary, cpu.stderr).groups()
        assert re.search(r"gpu: (\d+) partitions in \d+ passes, mark [\d.]+ ms; .* peak \d+ bytes", gpu.stderr).group(1) == parts
