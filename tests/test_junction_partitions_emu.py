"""The kernels of the PARTITIONED junction build (junctionInsertPart, junctionMarkPart, junctionFillMarked, junctionClassifyMarked in
sibeliaz_amd/csrc/lcb_junction_kernels.h) on the CPU wavefront emulator (tests/emu/junction_parts_emu.cpp): the unmodified device code,
driven like csrc/junctions.hip drives it - partition loop, regrowth of one partition's table, bitmap, table of junction k-mers, tiles -
writes the same junction file as lcb-mkgraph for every number of partitions. Logic only; the device runs are in
tests/test_gpu_junction_partitions.py."""
import os
import re
import subprocess

import pytest

from tests.test_junctions_emu import INPUTS as BASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
MKGRAPH = os.path.join(ROOT, "sibeliaz_amd", "bin", "lcb-mkgraph")


@pytest.fixture(scope="module")
def parts_emu(built):
    exe = os.path.join(EMU, "build", "junction_parts_emu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + EMU, "-I" + os.path.join(ROOT, "sibeliaz_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(EMU, "junction_parts_emu.cpp"), os.path.join(EMU, "emu_runtime.cpp")])
    return exe


def _inputs():
    k, _, _, iupac = BASE["iupac_one_tile"]
    assert (sum(len(s) + 1 for s in iupac.split("\n")[1::2]) + 1) % 64 != 0        # the last bitmap word is a partial one
    k31 = BASE["k31_strains_regrowth"]
    return {
        # name: (k, table_log2, tile_windows, FASTA text)
        "homopolymer": BASE["homopolymer"],                     # one partition holds everything, the others are empty
        "k3_random": BASE["k3_random"],                         # <= 32 keys: empty partitions at P = 7
        "k31_strains_log2_6": (k31[0], 6, k31[2], k31[3]),      # every partition's table has to grow, several times
        "no_window_records": BASE["no_window_records"],
        "iupac_tile64": (k, 20, 64, iupac),                     # tiles and bitmap words that cut records and N runs
        "iupac_tile777": (k, 20, 777, iupac),
    }


INPUTS = _inputs()
_cpu = {}


def run(parts_emu, name, tmp_path, partitions, max_log2=0):
    k, table_log2, tile, text = INPUTS[name]
    fa = str(tmp_path / "in.fa")
    with open(fa, "w") as f:
        f.write(text)
    if name not in _cpu:        # (the reference is computed once per input)
        cpu = str(tmp_path / "cpu.bin")
        subprocess.check_call([MKGRAPH, "-k", str(k), "-o", cpu, fa], stderr=subprocess.DEVNULL)
        _cpu[name] = open(cpu, "rb").read()
    emu = str(tmp_path / "emu.bin")
    r = subprocess.run([parts_emu, str(k), str(table_log2), str(tile), str(partitions), str(max_log2), emu, fa], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(emu, "rb").read() == _cpu[name]
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", r.stderr)}


@pytest.mark.parametrize("partitions", [2, 3, 7])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_partitioned_kernels_write_the_cpu_tools_file(parts_emu, name, partitions, tmp_path):
    info = run(parts_emu, name, tmp_path, partitions)
    assert info["partitions"] == info["passes"] == partitions
    if name == "k31_strains_log2_6":
        assert info["rebuilds"] > partitions and info["slots_log2"] > 6
    if name == "k3_random":
        assert info["junction_slots_log2"] > INPUTS[name][1]        # the table of junction k-mers had to grow as well
    if name.startswith("iupac"):
        assert info["tiles"] > 1


def test_one_partition_through_the_bitmap_path(parts_emu, tmp_path):
    info = run(parts_emu, "k31_strains_log2_6", tmp_path, 1)
    assert info["passes"] == 1 and info["rebuilds"] >= 2


def test_a_partition_that_may_not_grow_is_split(parts_emu, tmp_path):
    """The table may not grow beyond 2^9 slots (the driver: twice the slots would not fit the budget): a partition too full for it is
    split in two, (M, r) = (2M, r) + (2M, r + M), and the file stays the same."""
    info = run(parts_emu, "k31_strains_log2_6", tmp_path, 2, max_log2=9)
    assert info["passes"] > 2 and info["slots_log2"] == 9
