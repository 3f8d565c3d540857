"""The resource owner of the device layer (csrc/lcb_owned.h: every allocation, stream and event of a device is registered where it
is made and released from the registration) as plain C++ with stub allocate / free functions in place of the hip* calls:
tests/emu/owned_emu.cpp. Registering and releasing, re-registering a buffer that grows, and a creation that throws after the k-th
allocation for every k: each allocation is freed exactly once. The same program runs a second time under the address and
undefined-behaviour sanitizers (a stand-alone executable, nothing preloaded; a toolchain that cannot build it fails the test)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
SRC = os.path.join(EMU_DIR, "owned_emu.cpp")
FLAGS = ["-g", "-std=c++17", "-Wall", "-I" + CSRC]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(out_dir, extra):
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "owned_emu")
    deps = [SRC, os.path.join(CSRC, "lcb_owned.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++"] + extra + FLAGS + ["-o", exe, SRC])
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "every allocation released exactly once" in r.stdout
    assert int(r.stdout.split()[1]) >= 18


def test_every_allocation_is_released_once():
    _run(_build(os.path.join(EMU_DIR, "build"), ["-O2"]))


def test_every_allocation_is_released_once_sanitized():
    _run(_build(os.path.join(EMU_DIR, "build_san"), ["-O1"] + SANITIZE))
