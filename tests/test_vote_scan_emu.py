"""Stage A's pure parts of the look-ahead vote (lcb_used_fetch8 / lcb_used_first in csrc/lcb_kernel.h: the bitmap words of a voter's
window, the first used step in them) as functions of their own against the definition, a bit-by-bit loop over lcb_used_bit:
tests/emu/vote_scan_emu.cpp, built with g++ over the emulator's hip/hip_runtime.h, tiny pages (-DLCB_PAGE_SHIFT=2u) so that a view's
page table is exercised. Origins at word and page boundaries and at both ends of the map, both directions and strands (with the
- strand walking down onto the chromosome's first position), window lengths around every multiple of 32 / 64 and past the 225 steps
the eight words cover, no / one / random used bits. The same program runs a second time under the address and
undefined-behaviour sanitizers (a stand-alone executable, nothing preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
SRC = os.path.join(EMU_DIR, "vote_scan_emu.cpp")
FLAGS = ["-g", "-std=c++17", "-DLCB_PAGE_SHIFT=2u", "-I" + EMU_DIR, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(out_dir, name, extra):
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, name)
    deps = [SRC, os.path.join(CSRC, "lcb_kernel.h"), os.path.join(EMU_DIR, "hip", "hip_runtime.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++"] + extra + FLAGS + ["-o", exe, SRC])
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cases, all equal to the definition" in r.stdout
    assert int(r.stdout.split()[1]) > 100000


def test_scan_equals_the_definition():
    _run(_build(os.path.join(EMU_DIR, "build"), "vote_scan_emu", ["-O2"]))


def test_scan_equals_the_definition_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ cannot link the sanitizer runtimes")
    _run(_build(os.path.join(EMU_DIR, "build_san"), "vote_scan_emu", ["-O1"] + SANITIZE))
