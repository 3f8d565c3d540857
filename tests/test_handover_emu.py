"""The kernels of the hand-over route (sibeliaz_amd/csrc/lcb_handover_kernels.h) on the CPU wavefront emulator (tests/emu): the unmodified
device code, run behind the emulated table kernels as csrc/tables.hip runs it for lcb_open_fasta, fed the graph lcb_graph_load_impl makes
of a junction file written by the CPU lcb-mkgraph, gives back that graph's own host CSR - occChr, the widened payload = occG, the widened
scan = occStart -, the host's compactSmall decision, and, from a posCh seeded with the graph build's sentinel plus the patch list, the
loader's posCh at the device indices of a plan with seg_cap 64 and seg_gap 64 (an input of more than 32 * 64 positions in small
chromosomes has no such plan - lcb_plan_segments refuses more than 32 segments, as it does for a device: the emulator doubles the cap
until a plan exists and reports it). Every input runs with 32-bit and with 64-bit payloads
(one invocation of the emulator does both). Logic only; the parity tests proper are tests/test_gpu_handover.py on the MI355X."""
import os
import random
import re
import subprocess

import pytest

from tests import edge_inputs, seed_inputs, table_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")


@pytest.fixture(scope="module")
def handover_emu(built):
    exe = os.path.join(EMU, "build", "handover_emu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + EMU, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(EMU, "handover_emu.cpp"), os.path.join(CSRC, "graph.cpp"), os.path.join(EMU, "emu_runtime.cpp")])
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("handover_emu")


def _run(exe, graph, fasta, k, abundance):
    r = subprocess.run([exe, graph, str(k), str(abundance)] + list(fasta), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) (\d+)", r.stdout.strip().splitlines()[-1])}


@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_emulated_handover_matches_the_loader_on_edge_inputs(handover_emu, tmp, name):
    c = edge_inputs.build(name, str(tmp))
    out = _run(handover_emu, c["graph"], c["fasta"], c["k"], c["a"])
    assert out["vertices"] > 0
    if name == "all_filtered":
        assert 0 < out["positions"] < 64
    if name == "iupac_lowercase":
        assert out["patches"] > 0, "no junction in front of an IUPAC letter: handPatch did not run"


def emptied_text():
    """Three records; the middle one is 30 tandem copies of 16 bases: its only junctions are its first and its last window, whose k-mers
    occur 30 times each, so abundance 20 leaves it without a position (chrStart[2] == chrStart[1]) between two records that keep theirs."""
    rng = random.Random(3)
    s = "".join(rng.choice("ACGT") for _ in range(6000))
    r = "".join(rng.choice("ACGT") for _ in range(16))
    t = "".join((rng.choice("ACGT") if rng.random() < 0.1 else c) for c in s)
    return ">a\n%s\n>mid\n%s\n>b\n%s\n" % (s, r * 30, t)


def test_emulated_handover_never_answers_an_emptied_chromosome(handover_emu, tmp):
    graph, fasta = seed_inputs.write_input(tmp, "emptied", emptied_text())
    out = _run(handover_emu, graph, [fasta], seed_inputs.K, 20)
    assert out["emptied"] == 1 and out["positions"] > 256 and out["chromosomes"] == 3
    # ... and a synthetic junction file with an emptied chromosome between chromosomes of one position and of a sort tile
    c = table_inputs.write(tmp, "both_signs", table_inputs.TILE + 1)
    out = _run(handover_emu, c["graph"], [c["fasta"]], c["k"], c["a"])
    assert out["emptied"] == 1 and out["positions"] == c["positions"] and out["segments"] > 2


@pytest.mark.parametrize("params", seed_inputs.HEAVY)
def test_emulated_handover_matches_the_loader_on_heavy_inputs(handover_emu, tmp, params):
    graph, fasta = seed_inputs.heavy(tmp, *params)
    out = _run(handover_emu, graph, [fasta], seed_inputs.K, seed_inputs.ABUNDANCE)
    assert out["positions"] > params[0] and out["chromosomes"] == params[1] and out["segments"] > 1
    assert out["cap"] == 64 or out["positions"] > 32 * out["cap"] // 2, "the cap was doubled further than the 32 segments ask for"
    if params[3]:
        assert out["patches"] > 0
    if params[0] >= 257:
        assert out["small"] == 0, "lists of hundreds of occurrences: the large pools"


def test_emulated_handover_matches_the_loader_on_the_filtered_case(handover_emu, tmp):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp, *params)
    full = _run(handover_emu, graph, [fasta], seed_inputs.K, seed_inputs.ABUNDANCE)
    kept = _run(handover_emu, graph, [fasta], seed_inputs.K, abundance)
    assert 0 < kept["positions"] < full["positions"], "the abundance filter does not bite"


def test_emulated_handover_of_an_input_without_a_kept_position(handover_emu, tmp):
    graph, fasta = seed_inputs.heavy(tmp, *seed_inputs.HEAVY[0])
    out = _run(handover_emu, graph, [fasta], seed_inputs.K, 1)          # abundance 1: no count is below it
    assert out["positions"] == 0 and out["vertices"] > 0 and out["chromosomes"] == 3 and out["patches"] == 0
