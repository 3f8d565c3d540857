"""The kernels of the device seed enumeration (sibeliaz_amd/csrc/lcb_seed_kernels.h) on the CPU wavefront emulator (tests/emu): the unmodified
device code, driven like csrc/seeds.hip drives it (count, scan, fill, radix sort) over tables laid out as csrc/device.hip lays them out,
gives the host enumerator's seeds field by field and in order - on goldens, on lists that span several 64-occurrence chunks, on a
filtered CSR, on segmented tables with a gap, and on an input without a seed. Plus the sort kernels alone on generated keys. Logic only;
the parity tests proper are tests/test_gpu_seeds.py on the MI355X."""
import gzip
import os
import re
import subprocess

import pytest

from tests import seed_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TILE = 1024          # S_TILE of lcb_seed_kernels.h: the records of one workgroup of the scatter kernel (the harness prints it; checked below)
# seedScan32 walks the 256 histogram entries per tile in pieces of 4096: from 17 tiles on it takes a second piece (with exactly 17 the
# piece boundary falls inside one digit's run of the digit-major array), 34 tiles take three
SORT_SIZES = [0, 1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 16 * TILE, 16 * TILE + 1, 33 * TILE + 17]
PATTERNS = ["random", "count_top", "chr_only", "rank_low", "rank_wrap", "count_equal"]


@pytest.fixture(scope="module")
def seeds_emu(built):
    exe = os.path.join(EMU, "build", "seeds_emu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + EMU, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(EMU, "seeds_emu.cpp"), os.path.join(CSRC, "graph.cpp"), os.path.join(CSRC, "bundles.cpp"), os.path.join(EMU, "emu_runtime.cpp")])
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("seeds_emu")


def _golden(tmp, name):
    import json
    meta = json.load(open(os.path.join(GOLDEN, name, "golden.json")))
    out = {}
    for src, dst in (("genomes.fa.gz", name + ".fa"), ("graph.bin.gz", name + ".bin")):
        out[src] = os.path.join(str(tmp), dst)
        with gzip.open(os.path.join(GOLDEN, name, src), "rb") as f, open(out[src], "wb") as g:
            g.write(f.read())
    return out["graph.bin.gz"], out["genomes.fa.gz"], meta["k"], meta["a"]


def _run(exe, graph, fasta, k, a, *seg):
    r = subprocess.run([exe, "enum", graph, fasta, str(k), str(a)] + [str(x) for x in seg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) (\d+)", r.stdout)}


@pytest.mark.parametrize("name", ["smallb", "inv_k25"])
def test_emulated_enumeration_matches_host_on_goldens(seeds_emu, tmp, name):
    graph, fasta, k, a = _golden(tmp, name)
    out = _run(seeds_emu, graph, fasta, k, a)
    assert out["seeds"] > 0


@pytest.mark.parametrize("params", seed_inputs.HEAVY, ids=lambda p: "heavy_%d_%d_%d_%d" % p)
def test_emulated_enumeration_matches_host_on_long_lists(seeds_emu, tmp, params):
    graph, fasta = seed_inputs.heavy(tmp, *params)
    out = _run(seeds_emu, graph, fasta, seed_inputs.K, seed_inputs.ABUNDANCE)
    assert out["max_count"] >= params[0], "the generator no longer gives a list of %d occurrences: %r" % (params[0], out)


def test_emulated_enumeration_matches_host_on_filtered_csr(seeds_emu, tmp):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp, *params)
    out = _run(seeds_emu, graph, fasta, seed_inputs.K, abundance)
    assert 64 < out["max_count"] < params[0], "the abundance filter does not bite: %r" % (out,)


def test_emulated_enumeration_of_an_input_without_seeds(seeds_emu, tmp):
    graph, fasta = seed_inputs.no_seed(tmp)
    out = _run(seeds_emu, graph, fasta, seed_inputs.K, seed_inputs.ABUNDANCE)
    assert out["seeds"] == 0 and out["vertices"] > 0


def test_emulated_enumeration_on_segments_with_a_gap(seeds_emu, tmp):
    graph, fasta, k, a = _golden(tmp, "smallb")
    out = _run(seeds_emu, graph, fasta, k, a, 2000, 70001)
    assert out["segments"] > 1 and out["seeds"] > 0


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SORT_SIZES)
def test_emulated_sort_matches_std_sort(seeds_emu, n, pattern):
    r = subprocess.run([seeds_emu, "sort", str(n), pattern], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) (\d+)", r.stdout)}
    assert out["tile"] == TILE
    assert out["passes"] + out["skipped"] == 19
    if pattern == "count_equal":
        assert out["skipped"] >= 4, "every key has the same count: its four digits must be skipped (%r)" % (out,)
    if pattern in ("count_top", "rank_low") and n > 2:
        assert out["passes"] == 1, out
