"""Every one-workgroup scan kernel of the device-building routes alone on the CPU wavefront emulator (tests/emu, the `scan` mode of
seeds_emu, tables_emu, graph_emu and junction_emu): the unmodified kernel on a generated array, every output entry and the total against
a serial 64-bit prefix sum written in the harness (tests/emu/scan_cases.h).

The kernels that walk their array in pieces of 4 * 1024 entries, four per lane (seedScan32, tableScan32/64, graphScan), run at sizes
around one, two and three pieces and at sixteen pieces and one entry: the carry between pieces, the reuse of the wavefront sums in LDS
and the barrier that protects that reuse. The kernels that give every lane a run of `per` consecutive entries (seedScan64 =
seedScanBody, junctionScan) run around per = 1, 2, 3 and at 16, 17. junctionScan scans two tiles in a row through one JState; totJ,
totF, tileIdBase and idNext are checked after each.

Contents: all ones; random in [0, 1024] (a tile-histogram entry); random in [0, 256] with runs of zeros (blockKept with emptied
blocks); one non-zero entry at the first, the last and the first-of-second-piece index; and, for the 64-bit kernels, entries just below
2^31 so that the total and the sums of whole wavefronts pass 2^32 (the harness asserts that the serial total does; from three entries
on, since two entries below 2^31 cannot). One process per (kernel, size, schedule) runs every content.

Every case runs under the emulator's three schedules: wave 0 first with maximal skew, EMU_SCHED=rr (the waves take turns) and
EMU_SCHED=rev (the last wave first). The same programs run a second time under the address and undefined-behaviour sanitizers
(stand-alone executables, nothing preloaded). Logic only; the device tests are tests/test_gpu_scan_pieces.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
PIECE = 4096         # 4 * S_SCAN_T = 4 * T_SCAN_T = 4 * G_SCAN_T entries
PIECE_SIZES = [0, 1, 3, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1, 3 * PIECE + 17, 16 * PIECE + 1]
RUN_SIZES = [0, 1, 1023, 1024, 1025, 2047, 2049, 2735, 16384, 16385]
SCHEDULES = ["default", "rr", "rev"]
# kernel: (harness, arguments in front of the size, sizes, 64-bit entries)
KERNELS = {
    "seedScan32": ("seeds_emu", ["scan", "seedScan32"], PIECE_SIZES, False),
    "tableScan32": ("tables_emu", ["scan", "tableScan32"], PIECE_SIZES, False),
    "tableScan64": ("tables_emu", ["scan", "tableScan64"], PIECE_SIZES, True),
    "graphScan": ("graph_emu", ["scan"], PIECE_SIZES, True),
    "seedScan64": ("seeds_emu", ["scan", "seedScan64"], RUN_SIZES, True),
    "junctionScan": ("junction_emu", ["scan"], RUN_SIZES, False),
}
SOURCES = {
    "seeds_emu": ["seeds_emu.cpp", os.path.join(CSRC, "graph.cpp"), os.path.join(CSRC, "bundles.cpp"), "emu_runtime.cpp"],
    "tables_emu": ["tables_emu.cpp", os.path.join(CSRC, "graph.cpp"), "emu_runtime.cpp"],
    "graph_emu": ["graph_emu.cpp", os.path.join(CSRC, "graph.cpp"), "emu_runtime.cpp"],
    "junction_emu": ["junction_emu.cpp", "emu_runtime.cpp"],
}
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
CASES = [(k, n) for k in KERNELS for n in KERNELS[k][2]]


def _compile(out_dir, name, extra):
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, name)
    subprocess.check_call(["g++"] + extra + ["-std=c++17", "-fopenmp", "-I" + EMU, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe] +
                          [os.path.join(EMU, s) for s in SOURCES[name]])
    return exe


@pytest.fixture(scope="module")
def harness(built):
    return {name: _compile(os.path.join(EMU, "build"), name, ["-O2"]) for name in SOURCES}


def _contents(n, wide):
    return ["ones", "hist", "kept", "first", "last", "second"] + (["big"] if wide and n >= 3 else [])


def _run(exe, kernel, n, sched, **extra):
    _, args, _, wide = KERNELS[kernel]
    env = dict({k: v for k, v in os.environ.items() if k != "EMU_SCHED"}, **extra)
    if sched != "default":
        env["EMU_SCHED"] = sched
    r = subprocess.run([exe] + args + [str(n)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("scan " + kernel + " ")]
    return lines, wide


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("kernel,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_scan_kernel_equals_the_serial_prefix_sum(harness, kernel, n, sched):
    lines, wide = _run(harness[KERNELS[kernel][0]], kernel, n, sched)
    if kernel == "junctionScan":
        # scan junctionScan nb N per P <content> tile T totJ A totF B: two tiles per content
        assert [(ln[6], int(ln[8])) for ln in lines] == [(c, t) for c in _contents(n, wide) for t in (0, 1)]
        assert all(int(ln[3]) == n and int(ln[5]) == (n + 1023) // 1024 for ln in lines)
        ones = [ln for ln in lines if ln[6] == "ones"]
        assert all(int(ln[10]) == int(ln[12]) == n for ln in ones)
        return
    # scan <kernel> n N <content> total T
    assert [ln[4] for ln in lines] == _contents(n, wide), "a content did not run"
    assert all(int(ln[3]) == n for ln in lines)
    totals = {ln[4]: int(ln[6]) for ln in lines}
    assert totals["ones"] == n
    for c in ("first", "last", "second"):
        assert totals[c] == (1000 if n else 0)
    if "big" in totals:
        assert totals["big"] > 1 << 32


def test_sizes_reach_the_pieces_they_are_meant_for():
    """The size lists against the constants of the kernel headers: a change of the lane count or of the entries per lane must move them."""
    text = {h: open(os.path.join(CSRC, h)).read() for h in ("lcb_seed_kernels.h", "lcb_table_kernels.h", "lcb_graph_kernels.h", "lcb_junction_kernels.h")}
    for header, name in (("lcb_seed_kernels.h", "S_SCAN_T"), ("lcb_table_kernels.h", "T_SCAN_T"), ("lcb_graph_kernels.h", "G_SCAN_T")):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, text[header]).group(1)) * 4 == PIECE
        assert "p0 += 4ull * %s" % name in text[header]
    assert "__launch_bounds__(1024) void junctionScan" in text["lcb_junction_kernels.h"] and "per = (nb + 1023) / 1024" in text["lcb_junction_kernels.h"]
    pieces = sorted({(n + PIECE - 1) // PIECE for n in PIECE_SIZES})
    assert pieces == [0, 1, 2, 3, 4, 17]
    assert sorted({(n + 1023) // 1024 for n in RUN_SIZES}) == [0, 1, 2, 3, 16, 17]


@pytest.fixture(scope="module")
def sanitized(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_san")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + ["-o", str(tmp / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ cannot link the sanitizer runtimes")
    return {name: _compile(os.path.join(EMU, "build_san"), name, ["-O1", "-g"] + SANITIZE) for name in SOURCES}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_scan_kernel_under_the_sanitizers(sanitized, kernel):
    """Sizes around the second piece / the second entry per lane, where an index past the array would first show. (No leak check: the
    emulator's runtime keeps the stacks of its lanes until the process ends.)"""
    for n in ((PIECE - 1, 2 * PIECE + 1) if KERNELS[kernel][2] is PIECE_SIZES else (1023, 2049)):
        lines, wide = _run(sanitized[KERNELS[kernel][0]], kernel, n, "default", ASAN_OPTIONS="detect_leaks=0")
        assert len(lines) == len(_contents(n, wide)) * (2 if kernel == "junctionScan" else 1)
