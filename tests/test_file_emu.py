"""The kernels that open a junction file on the GPU (sibeliaz_amd/csrc/lcb_file_kernels.h) on the CPU wavefront emulator (tests/emu): the
unmodified device code and the unmodified tail of the graph build (lcb_graph_kernels.h), driven by tests/emu/file_emu.cpp as graphFromFile
and graphTail of csrc/junctions.hip drive them, with the host code they use (lcb_file_host.h), give the graph lcb_graph_load_impl makes
of the same files - chrStart, the four per-position arrays, nVertex and the host CSR - or the loader's refusal, word for word: on the
edge inputs, every heavy input of tests/seed_inputs.py and the filtered case at tiles of 64, 777 and 4096 records, and on the
hand-packed files of tests/file_inputs.py at tiles of 64. The host code alone runs once more as a stand-alone program under
AddressSanitizer and UBSan. Logic only; the parity tests proper are tests/test_gpu_file_open.py on the MI355X."""
import os
import re
import subprocess

import pytest

from tests import edge_inputs, file_inputs, seed_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
TILES = (64, 777, 4096)


@pytest.fixture(scope="module")
def file_emu(built):
    exe = os.path.join(EMU, "build", "file_emu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + EMU, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(EMU, "file_emu.cpp"), os.path.join(CSRC, "graph.cpp"), os.path.join(EMU, "emu_runtime.cpp")])
    return exe


@pytest.fixture(scope="module")
def host_check(built):
    exe = os.path.join(EMU, "build", "file_host_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(EMU, "file_host_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("file_emu")


def _numbers(line):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) (\d+)", line)}


def _run(exe, graph, fasta, k, abundance, tile):
    r = subprocess.run([exe, graph, str(k), str(abundance), str(tile)] + list(fasta), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = r.stdout.strip().splitlines()[-1]
    assert not line.startswith("refused"), line
    out = _numbers(line)
    assert out["kept"] <= out["raw"] == out["records"] - out["separators"]
    per = max(1, min(tile, out["records"]))
    assert out["tiles"] == (out["records"] + per - 1) // per
    return out


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_emulated_file_matches_the_loader_on_edge_inputs(file_emu, tmp, name, tile):
    c = edge_inputs.build(name, str(tmp))
    out = _run(file_emu, c["graph"], c["fasta"], c["k"], c["a"], tile)
    assert out["raw"] > 0 and out["chromosomes"] >= 1
    if name in ("multi_file", "small_b_large_m"):    # (the others may have a handful of junctions)
        assert tile > 64 or out["tiles"] > 1
    if name == "all_filtered":
        assert 0 < out["kept"] < out["raw"] // 2
    if name == "iupac_lowercase":
        assert out["patched"] > 0, "no junction in front of an IUPAC letter: the sentinel patch did not run"


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("params", seed_inputs.HEAVY)
def test_emulated_file_matches_the_loader_on_heavy_inputs(file_emu, tmp, params, tile):
    graph, fasta = seed_inputs.heavy(tmp, *params)
    out = _run(file_emu, graph, [fasta], seed_inputs.K, seed_inputs.ABUNDANCE, tile)
    assert out["kept"] == out["raw"] > params[0] and out["chromosomes"] == params[1]
    if params[3]:
        assert out["patched"] > 0


@pytest.mark.parametrize("tile", TILES)
def test_emulated_file_matches_the_loader_on_the_filtered_case(file_emu, tmp, tile):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp, *params)
    out = _run(file_emu, graph, [fasta], seed_inputs.K, abundance, tile)
    assert 0 < out["kept"] < out["raw"], "the abundance filter does not bite"


def _property(name, c, out):
    """What the case stands for, asserted on the file itself and on the counts the run printed."""
    data = open(c["graph"], "rb").read()
    n = len(data) // 12
    recs = [(int.from_bytes(data[12 * r:12 * r + 4], "little"), int.from_bytes(data[12 * r + 4:12 * r + 12], "little", signed=True)) for r in range(n)]
    sep = [p == 0xFFFFFFFF or i == file_inputs.INT64_MAX for p, i in recs]
    assert out["records"] == n and out["separators"] == sum(sep) == c["separators"] and out["chromosomes"] == len(c["sizes"]) and out["raw"] == sum(c["sizes"])
    T = file_inputs.TILE
    if name == "signed_ids":
        assert any(i < 0 for (p, i), s in zip(recs, sep) if not s)
    if name == "high_bits":
        assert all(i >> 32 not in (0, -1) for (p, i), s in zip(recs, sep) if not s)
    if name == "separators_either_way":
        assert any(p == 0xFFFFFFFF and i != file_inputs.INT64_MAX for p, i in recs) and any(p != 0xFFFFFFFF and i == file_inputs.INT64_MAX for p, i in recs)
    if name == "no_trailing_separator":
        assert not sep[-1]
    if name == "three_trailing_separators":
        assert sep[-3:] == [True] * 3 and not sep[-4]
    if name == "stray_bytes":
        assert len(data) % 12 == 5
    if name == "sparse_ids":
        distinct = {abs(i) for (p, i), s in zip(recs, sep) if not s}
        assert out["vertices"] == max(distinct) + 1 == 10 * len(distinct) + 1
    if name == "long_chromosome":
        assert max(c["sizes"]) > 20 * T
    if name == "all_filtered":
        assert out["kept"] == 0 < out["raw"]
    if name == "filtered_beyond_end":
        assert out["kept"] == out["raw"] - 4
    if name == "tile_edges":
        assert sep[T - 1] and sep[2 * T] and not sep[2 * T - 1] and all(sep[3 * T:4 * T]) and n > 4 * T
    if name in ("separators_only", "empty"):
        assert out["raw"] == out["vertices"] == out["chromosomes"] == 0 and (out["separators"] > 0) == (name == "separators_only")
    elif name != "all_filtered":
        assert out["kept"] > 0 and n >= 4 * T


@pytest.mark.parametrize("name", file_inputs.LEGAL)
def test_emulated_file_matches_the_loader_on_hand_packed_files(file_emu, tmp, name):
    c = file_inputs.build(name, tmp)
    out = _run(file_emu, c["graph"], c["fasta"], c["k"], c["a"], file_inputs.TILE)
    _property(name, c, out)


@pytest.mark.parametrize("name", sorted(file_inputs.ERRORS))
def test_emulated_file_is_refused_with_the_loaders_words(file_emu, tmp, name):
    c = file_inputs.build(name, tmp)
    r = subprocess.run([file_emu, c["graph"], str(c["k"]), str(c["a"]), str(file_inputs.TILE)] + c["fasta"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr              # (0: the loader and the emulated route refuse with the same text)
    assert r.stdout.strip().splitlines()[-1] == "refused: " + c["error"]


@pytest.mark.parametrize("tile", (file_inputs.TILE, 777))
@pytest.mark.parametrize("name", file_inputs.NAMES)
def test_host_part_under_the_sanitizers(host_check, tmp, name, tile):
    c = file_inputs.build(name, tmp)
    n_fasta = open(c["fasta"][0]).read().count(">")
    r = subprocess.run([host_check, c["graph"], str(tile), str(n_fasta)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    line = r.stdout.strip()
    if name in ("err_empty_run", "err_fasta_more", "err_fasta_fewer"):          # (the other two defects are the kernels' to find)
        assert line == "refused: " + c["error"]
        return
    out = _numbers(line)
    n = os.path.getsize(c["graph"]) // 12
    per = max(1, min(tile, n))
    assert out["records"] == n and out["separators"] == c["separators"] and out["raw"] == sum(c["sizes"]) and out["chromosomes"] == len(c["sizes"])
    assert out["tiles"] == (n + per - 1) // per and out["blocks"] == out["tiles"] * ((per + 255) // 256)
