"""The partitioned junction build's surface that needs no GPU: the layouts of lcb_junction_opts_ex / lcb_junction_stats_ex, the planner
(lcb_junctions_plan: pure arithmetic - how many partitions fit a budget of device memory), the argument checks of
lcb_junctions_build_ex (made before the device is touched), and the loud failures of `build_junctions(partitions=...)` and of
`lcb-mkgraph --gpu --partitions` on a machine without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sibeliaz_amd
from sibeliaz_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MKGRAPH = os.path.join(ROOT, "sibeliaz_amd", "bin", "lcb-mkgraph")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.fixture
def fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_text(">a\nACGTTGCAAGGCTTACGATCGATTTACGGCATCGA\n>b\nACGTTGCAAGGCTTACGTTCGATTTACGGCATCGA\n")
    return str(p)


def _no_file(out):
    assert not os.path.exists(out) and not os.path.exists(out + ".part")


def test_ex_structs_have_the_layout_of_the_header(built, tmp_path):
    opts = ["abi", "table_log2", "tile_windows", "partitions", "mem_budget", "reserved"]
    stats = ["base", "partitions", "junction_windows", "junction_table_slots", "peak_device_bytes", "mark_ms", "passes"]
    args = ["sizeof(lcb_junction_opts_ex)", "sizeof(lcb_junction_stats_ex)"] + ["offsetof(lcb_junction_opts_ex, %s)" % f for f in opts] + [
        "offsetof(lcb_junction_stats_ex, %s)" % f for f in stats] + ["sizeof(lcb_junction_stats)"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lcb.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n'
                   % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(api.JunctionOptsEx), C.sizeof(api.JunctionStatsEx)] + [getattr(api.JunctionOptsEx, f).offset for f in opts] + [
        getattr(api.JunctionStatsEx, f).offset for f in stats] + [C.sizeof(api.JunctionStats)]
    assert got == want
    assert api.JunctionStatsEx.base.offset == 0 and api.JunctionStatsEx.partitions.offset == C.sizeof(api.JunctionStats)
    L = sibeliaz_amd.load_library()
    assert L.lcb_abi_version() == 6
    for name in ("lcb_junctions_build_ex", "lcb_junctions_plan"):
        assert name in api.EXPORTS and hasattr(L, name)


# ---- the planner

def _need(windows, seq_bytes, partitions, table_log2=0):
    """The formula of DESIGN.md §10, written down independently of the library."""
    slots = 1 << table_log2 if table_log2 else 1 << 20
    while not table_log2 and slots < windows // (2 * partitions):
        slots *= 2
    return seq_bytes + 8 * ((seq_bytes + 63) // 64) + 12 * slots + 64


def test_plan_one_partition_when_the_budget_is_generous(built):
    assert sibeliaz_amd.plan_junctions(10 ** 7, 10 ** 7 + 9, 1 << 40) == (1, _need(10 ** 7, 10 ** 7 + 9, 1))
    assert sibeliaz_amd.plan_junctions(0, 1, 1 << 30) == (1, _need(0, 1, 1))


def test_plan_need_follows_the_formula_and_never_grows_with_the_partitions(built):
    for windows in (5 * 10 ** 6, 3 * 10 ** 9, 44 * 10 ** 9):
        needs = []
        for p in range(1, 65):
            got_p, need = sibeliaz_amd.plan_junctions(windows, windows + 17, 0, partitions=p)
            assert got_p == p and need == _need(windows, windows + 17, p)
            needs.append(need)
        assert all(a >= b for a, b in zip(needs, needs[1:])) and needs[0] > needs[-1]
    # a fixed table size is a fixed need
    assert {sibeliaz_amd.plan_junctions(10 ** 9, 10 ** 9, 0, partitions=p, table_log2=24)[1] for p in (1, 7, 64)} == {_need(10 ** 9, 10 ** 9, 1, 24)}


def test_plan_44_gbp_on_one_mi355x(built):
    windows, seq, budget = 44 * 10 ** 9, 44 * 10 ** 9 + 1, 288 * 10 ** 9
    p, need = sibeliaz_amd.plan_junctions(windows, seq, budget)
    assert p > 1 and need <= budget
    assert need == _need(windows, seq, p) and _need(windows, seq, p - 1) > budget        # the smallest that fits
    assert sibeliaz_amd.plan_junctions(windows, seq, budget, partitions=1)[1] > budget


def test_plan_impossible_budget_names_both_numbers(built):
    windows, seq = 10 ** 8, 10 ** 8 + 1
    budget = seq // 2           # (less than the sequence itself)
    with pytest.raises(sibeliaz_amd.LcbError) as e:
        sibeliaz_amd.plan_junctions(windows, seq, budget)
    assert str(_need(windows, seq, 64)) in str(e.value) and str(budget) in str(e.value)


def test_plan_refuses_65_partitions_and_another_abi(built):
    with pytest.raises(sibeliaz_amd.LcbError, match="at most 64"):
        sibeliaz_amd.plan_junctions(10 ** 6, 10 ** 6, 1 << 40, partitions=65)
    with pytest.raises(sibeliaz_amd.LcbError, match="LCB_ABI_VERSION"):
        sibeliaz_amd.plan_junctions(10 ** 6, 10 ** 6, 1 << 40, abi=5)
    with pytest.raises(sibeliaz_amd.LcbError, match="negative"):
        sibeliaz_amd.plan_junctions(-1, 10 ** 6, 1 << 40)
    with pytest.raises(TypeError):
        sibeliaz_amd.plan_junctions(10 ** 6, 10 ** 6, 1 << 40, bogus=1)


# ---- lcb_junctions_build_ex: what can be refused without a device is refused before the device is touched (these pass on any machine)

@pytest.mark.parametrize("kw,match", [
    (dict(partitions=65), "at most 64"),
    (dict(partitions=2, abi=5), "LCB_ABI_VERSION"),
    (dict(partitions=2, table_log2=41), "table_log2"),
    (dict(mem_budget=1 << 30, tile_windows=(1 << 30) + 1), "tile_windows"),
])
def test_ex_option_errors_come_before_the_device(built, fasta, tmp_path, kw, match):
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match=match):
        sibeliaz_amd.build_junctions([fasta], 15, out, **kw)
    _no_file(out)


def test_ex_argument_errors_come_before_the_device(built, fasta, tmp_path):
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match="k must be odd"):
        sibeliaz_amd.build_junctions([fasta], 24, out, partitions=2)
    with pytest.raises(sibeliaz_amd.LcbError, match="no FASTA file"):
        sibeliaz_amd.build_junctions([], 15, out, partitions=2)
    with pytest.raises(sibeliaz_amd.LcbError, match="cannot open"):
        sibeliaz_amd.build_junctions([fasta, str(tmp_path / "absent.fa")], 15, out, mem_budget=1 << 30)
    with pytest.raises(TypeError):
        sibeliaz_amd.build_junctions([fasta], 15, out, partitions=2, bogus=1)
    _no_file(out)


def test_partitioned_build_fails_loudly_without_gpu(built, fasta, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is present")
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match="no CPU fallback"):
        sibeliaz_amd.build_junctions([fasta], 15, out, partitions=2)
    _no_file(out)


def test_tool_partitions_flag_fails_loudly_without_gpu(built, fasta, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is present")
    out = str(tmp_path / "g.bin")
    env = {k: v for k, v in os.environ.items() if k != "LCB_LIB"}
    r = subprocess.run([MKGRAPH, "--gpu", "0", "--partitions", "2", "-k", "15", "-o", out, fasta], capture_output=True, text=True, env=env)
    assert r.returncode == 1
    assert "lcb-mkgraph: error:" in r.stderr and "no CPU fallback" in r.stderr
    _no_file(out)


def test_tool_usage_names_the_partition_flags(built, fasta, tmp_path):
    r = subprocess.run([MKGRAPH], capture_output=True, text=True)
    assert r.returncode == 2
    assert r.stderr.startswith("usage: lcb-mkgraph -k <odd 3..31> -o junctions.bin [--gpu <ordinal>")
    assert "--partitions" in r.stderr and "--mem-budget" in r.stderr
    # a number of partitions the library would refuse is a usage error of the tool
    r = subprocess.run([MKGRAPH, "--gpu", "0", "--partitions", "65", "-k", "15", "-o", str(tmp_path / "g.bin"), fasta], capture_output=True, text=True)
    assert r.returncode == 2 and re.search(r"--partitions <1\.\.64\|auto>", r.stderr)
    _no_file(str(tmp_path / "g.bin"))
