"""The kernels of the device table build (sibeliaz_amd/csrc/lcb_table_kernels.h) on the CPU wavefront emulator (tests/emu): the unmodified
device code, driven like csrc/tables.hip drives it (windows, keys + counts, scan, radix sort, gather) over inputs laid out as
csrc/device.hip lays them out, gives what the host route uploads - lcb_window_table, the graph's occStart, the occurrence records in
graph.cpp's order - on goldens, on every synthetic pattern of tests/table_inputs.py, on long lists and a filtered CSR, on segmented
tables with a gap (the 64-bit instantiation), on an input without a position, and on positions at both ends of the 32-bit range.
Logic only; the parity tests proper are tests/test_gpu_tables.py on the MI355X."""
import gzip
import json
import os
import re
import subprocess

import pytest

from tests import edge_inputs, seed_inputs, table_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
# tableScan walks the 256 histogram entries per tile in pieces of 4096: from 17 tiles on it takes a second piece (with exactly 17 the
# piece boundary falls inside one digit's run of the digit-major array), 34 tiles take three
SIZES = table_inputs.SIZES + [16 * table_inputs.TILE, 16 * table_inputs.TILE + 1, 33 * table_inputs.TILE + 17]


@pytest.fixture(scope="module")
def tables_emu(built):
    exe = os.path.join(EMU, "build", "tables_emu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + EMU, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(EMU, "tables_emu.cpp"), os.path.join(CSRC, "graph.cpp"), os.path.join(EMU, "emu_runtime.cpp")])
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tables_emu")


def _golden(tmp, name):
    meta = json.load(open(os.path.join(GOLDEN, name, "golden.json")))
    out = {}
    for src, dst in (("genomes.fa.gz", name + ".fa"), ("graph.bin.gz", name + ".bin")):
        out[src] = os.path.join(str(tmp), dst)
        with gzip.open(os.path.join(GOLDEN, name, src), "rb") as f, open(out[src], "wb") as g:
            g.write(f.read())
    return out["graph.bin.gz"], out["genomes.fa.gz"], meta["k"], meta["a"]


def _out(r):
    assert r.returncode == 0, r.stderr
    # (one line per build: the last one counts where a mode runs several)
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) (\d+)", r.stdout.strip().splitlines()[-1])}
    assert out["tile"] == table_inputs.TILE and out["passes"] + out["skipped"] == 4
    return out


def _run(exe, graph, fasta, k, a, max_branch, *seg):
    return _out(subprocess.run([exe, "graph", graph, fasta, str(k), str(a), str(max_branch)] + [str(x) for x in seg], capture_output=True, text=True))


@pytest.mark.parametrize("name", ["smallb", "inv_k25"])
def test_emulated_tables_match_host_on_goldens(tables_emu, tmp, name):
    graph, fasta, k, a = _golden(tmp, name)
    out = _run(tables_emu, graph, fasta, k, a, 50)
    assert out["positions"] > 0 and out["payload_bytes"] == 4


@pytest.mark.parametrize("max_branch", table_inputs.MAX_BRANCH)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", table_inputs.PATTERNS)
def test_emulated_tables_match_host_on_patterns(tables_emu, tmp, pattern, n, max_branch):
    c = table_inputs.write(tmp, pattern, n)
    out = _run(tables_emu, c["graph"], c["fasta"], c["k"], c["a"], max_branch)
    assert out["positions"] == n and out["vertices"] == c["vertices"] and out["chromosomes"] == c["chromosomes"]
    want = table_inputs.expected_passes(pattern, n)
    if want:
        assert (out["passes"], out["skipped"]) == want


def test_emulated_tables_on_a_pattern_cut_into_segments(tables_emu, tmp):
    c = table_inputs.write(tmp, "both_signs", table_inputs.SIZES[-1])
    out = _run(tables_emu, c["graph"], c["fasta"], c["k"], c["a"], 12, 1100, 70001)
    assert out["segments"] > 2 and out["payload_bytes"] == 8


def test_emulated_tables_match_host_on_long_lists_and_filtered_csr(tables_emu, tmp):
    graph, fasta = seed_inputs.heavy(tmp, *seed_inputs.HEAVY[3])
    assert _run(tables_emu, graph, fasta, seed_inputs.K, seed_inputs.ABUNDANCE, 200)["positions"] > 0
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp, *params)
    full = _run(tables_emu, graph, fasta, seed_inputs.K, seed_inputs.ABUNDANCE, 200)
    kept = _run(tables_emu, graph, fasta, seed_inputs.K, abundance, 200)
    assert 0 < kept["positions"] < full["positions"], "the abundance filter does not bite"


def test_emulated_tables_on_segments_with_a_gap(tables_emu, tmp):
    graph, fasta, k, a = _golden(tmp, "smallb")
    out = _run(tables_emu, graph, fasta, k, a, 50, 2000, 70001)
    assert out["segments"] > 1 and out["payload_bytes"] == 8


def test_emulated_tables_of_an_input_without_positions(tables_emu, tmp):
    c = table_inputs.all_filtered(tmp)
    out = _run(tables_emu, c["graph"], c["fasta"], c["k"], c["a"], 200)
    assert out["positions"] == 0 and out["vertices"] > 0 and out["chromosomes"] == 2 and out["passes"] == 0
    # edge_inputs' all_filtered keeps the junctions that occur once: a handful of positions, every list of length one
    c = edge_inputs.build("all_filtered", str(tmp))
    out = _run(tables_emu, c["graph"], c["fasta"][0], c["k"], c["a"], c["b"])
    assert 0 < out["positions"] < 64


@pytest.mark.parametrize("max_branch", [0, 3, 400, 64999])
def test_emulated_windows_saturate_at_both_ends_of_the_position_range(tables_emu, max_branch):
    out = _out(subprocess.run([tables_emu, "edge", str(max_branch)], capture_output=True, text=True))
    assert out["positions"] == 30 and out["segments"] > 1
