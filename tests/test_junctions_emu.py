"""The kernels of the GPU junction finder (sibeliaz_amd/csrc/lcb_junction_kernels.h) on the CPU wavefront emulator (tests/emu): the
unmodified device code, driven like csrc/junctions.hip drives it, writes the same junction file as lcb-mkgraph - with a table that
has to grow several times and with tiles that cut records, breakers and first appearances. Logic only; the parity tests proper are
tests/test_gpu_junctions.py on the MI355X."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
MKGRAPH = os.path.join(ROOT, "sibeliaz_amd", "bin", "lcb-mkgraph")


@pytest.fixture(scope="module")
def junction_emu(built):
    exe = os.path.join(EMU, "build", "junction_emu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + EMU, "-I" + os.path.join(ROOT, "sibeliaz_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(EMU, "junction_emu.cpp"), os.path.join(EMU, "emu_runtime.cpp")])
    return exe


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _inputs():
    rng = random.Random(11)
    a, b = _rand(rng, 400), _rand(rng, 300)
    s = _rand(rng, 2500)
    t = "".join((rng.choice("ACGT") if rng.random() < 0.02 else c) for c in s)
    return {
        # name: (k, table_log2, tile_windows, FASTA text)
        "no_window_records": (15, 20, 64, ">a\n%s\n>short\nACGTACG\n>empty\n>enn\n%s\n>b\n%s\n" % (a, "N" * 40, b + a[50:150])),
        "homopolymer": (15, 4, 1000, ">a\n%s\n>t\n%s\n" % ("A" * 3000, "T" * 3000)),
        "k3_random": (3, 3, 300, ">r\n%s\n" % _rand(rng, 2000)),
        "k31_strains_regrowth": (31, 8, 777, ">s\n%s\n>t\n%s\n" % (s, t)),
        "iupac_one_tile": (11, 20, 1 << 22, ">s\n%s\n>t\n%s\n" % (s[:900] + "NNRY" + s[900:1800].lower(), t[:1500])),
    }


INPUTS = _inputs()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_emulated_kernels_write_the_cpu_tools_file(junction_emu, name, tmp_path):
    k, table_log2, tile, text = INPUTS[name]
    fa = str(tmp_path / "in.fa")
    with open(fa, "w") as f:
        f.write(text)
    cpu, emu = str(tmp_path / "cpu.bin"), str(tmp_path / "emu.bin")
    subprocess.check_call([MKGRAPH, "-k", str(k), "-o", cpu, fa], stderr=subprocess.DEVNULL)
    subprocess.check_call([junction_emu, str(k), str(table_log2), str(tile), emu, fa], stderr=subprocess.DEVNULL)
    assert open(emu, "rb").read() == open(cpu, "rb").read()
