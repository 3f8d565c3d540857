"""The kernels of the graph build on the GPU (sibeliaz_amd/csrc/lcb_graph_kernels.h) on the CPU wavefront emulator (tests/emu): the
unmodified device code, driven like lcb_graph_build_impl of csrc/junctions.hip drives it behind the junction finder, fed the raw records
of a junction file written by the CPU lcb-mkgraph and the code bytes, gives the graph lcb_graph_load_impl makes of that file - chrStart,
the four per-position arrays, nVertex and the host CSR - on the edge inputs, on every heavy input of tests/seed_inputs.py, on the filtered
case, on an input without a kept position, at tile sizes 64, 777 and 4096. Logic only; the parity tests proper are
tests/test_gpu_graph_build.py on the MI355X."""
import os
import re
import subprocess

import pytest

from tests import edge_inputs, seed_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
TILES = (64, 777, 4096)


@pytest.fixture(scope="module")
def graph_emu(built):
    exe = os.path.join(EMU, "build", "graph_emu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + EMU, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(EMU, "graph_emu.cpp"), os.path.join(CSRC, "graph.cpp"), os.path.join(EMU, "emu_runtime.cpp")])
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("graph_emu")


def _run(exe, graph, fasta, k, abundance, tile):
    r = subprocess.run([exe, graph, str(k), str(abundance), str(tile)] + list(fasta), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) (\d+)", r.stdout.strip().splitlines()[-1])}
    assert out["kept"] <= out["raw"] and out["tiles"] >= 1
    return out


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_emulated_graph_matches_the_loader_on_edge_inputs(graph_emu, tmp, name, tile):
    c = edge_inputs.build(name, str(tmp))
    out = _run(graph_emu, c["graph"], c["fasta"], c["k"], c["a"], tile)
    assert out["raw"] > 0 and out["tiles"] > 1
    if name == "all_filtered":
        assert 0 < out["kept"] < out["raw"] // 2
    if name == "iupac_lowercase":
        assert out["patched"] > 0, "no junction in front of an IUPAC letter: the sentinel patch did not run"


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("params", seed_inputs.HEAVY)
def test_emulated_graph_matches_the_loader_on_heavy_inputs(graph_emu, tmp, params, tile):
    graph, fasta = seed_inputs.heavy(tmp, *params)
    out = _run(graph_emu, graph, [fasta], seed_inputs.K, seed_inputs.ABUNDANCE, tile)
    assert out["kept"] == out["raw"] > params[0] and out["records"] == params[1]
    if params[3]:
        assert out["patched"] > 0


@pytest.mark.parametrize("tile", TILES)
def test_emulated_graph_matches_the_loader_on_the_filtered_case(graph_emu, tmp, tile):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp, *params)
    out = _run(graph_emu, graph, [fasta], seed_inputs.K, abundance, tile)
    assert 0 < out["kept"] < out["raw"], "the abundance filter does not bite"


@pytest.mark.parametrize("tile", TILES)
def test_emulated_graph_of_an_input_without_a_kept_position(graph_emu, tmp, tile):
    graph, fasta = seed_inputs.heavy(tmp, *seed_inputs.HEAVY[0])
    out = _run(graph_emu, graph, [fasta], seed_inputs.K, 1, tile)          # abundance 1: no count is below it
    assert out["kept"] == 0 and out["raw"] > 0 and out["vertices"] > 0 and out["records"] == 3
