"""The resolved heavy vote of the wide and big variants (lcb_vote_resolve / lcb_vote_items in csrc/lcb_kernel.h) under the wavefront
emulator: one more harness binary - the sources and flags of tests/emu/build/emu_check_share8 plus tiny thresholds, so that every
multi-wavefront vote of 2 .. 72 voters takes the resolved path and larger ones fall back to the ticket walk - against the CPU oracle:
per-seed results, footprints (EMU_FP_CHECK) and event counters. tests/emu/emu_resolve_main.cpp adds the event counters of the
resolved path (they exist only in this build) and the wide / big modes with a `used` state to emu_check.

The synthetic input is bench.py's config 3 at 70 strains and 4 segments, lcb-synth seed 9101 (1.8 Mbp): votes of 65 .. 72 voters need
a second round of stage A, windows have several 64-step chunks, repeats give votes above the maximum. With runs of used positions
(`*-runs`) its first 30 seeds go through all of: an item of chunk >= 1, a `used` stop beyond step 64, a vote repeated after a path
hit, a vote above LCB_VOTE_RESOLVE_MAX that fell back, a second round of stage A (asserted below)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EXE = os.path.join(EMU_DIR, "build", "emu_check_resolve")
CSRC = os.path.join(ROOT, "sibeliaz_amd", "csrc")
SRC = [os.path.join(EMU_DIR, "emu_resolve_main.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")] + [os.path.join(CSRC, f) for f in ("graph.cpp", "bundles.cpp", "commit.cpp", "engine.cpp", "output.cpp")]
FLAGS = ["-O2", "-g", "-std=c++17", "-fopenmp", "-DLCB_VOTE_SHARE_MIN=2u", "-DLCB_PAGE_SHIFT=2u", "-DLCB_TEST_FP_SLOT_DIV=16u",      # as emu_check_share8
         "-DLCB_VOTE_RESOLVE_MIN=2u", "-DLCB_VOTE_RESOLVE_MAX=72u", "-DLCB_TEST_RESOLVE_EVENT=lcb_test_resolve_event"]
SYNTH = ("--strains 70 --segments 4 --keep 0.8 --swap 0.05 --invert 0.10 --sub 0.02 --indel 0.002 --filler-frac 0.25 --filler-min 200 --filler-max 3000 "
         "--repeat-families 3 --repeat-copies 10 --repeat-len 800 --seg-min 500 --seg-max 8000 --seed 9101")


@pytest.fixture(scope="module")
def emu_resolve(built):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "all"])           # (the oracle object and the stock harnesses, unchanged)
    deps = SRC + [os.path.join(EMU_DIR, "emu_main.cpp"), os.path.join(CSRC, "lcb_kernel.h"), os.path.join(EMU_DIR, "build", "lcb_oracle.o")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++"] + FLAGS + ["-I" + EMU_DIR, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", EXE] + SRC + [os.path.join(EMU_DIR, "build", "lcb_oracle.o")])
    return EXE


@pytest.fixture(scope="module")
def synth(built, tmp_path_factory):
    import bench
    d = tmp_path_factory.mktemp("vote_resolve_emu")
    fa, gr = str(d / "g.fa"), str(d / "g.bin")
    subprocess.check_call([os.path.join(bench.BIN, "lcb-synth"), "-o", fa] + SYNTH.split())
    subprocess.check_call([os.path.join(bench.BIN, "lcb-mkgraph"), "-k", "15", "-o", gr, fa], stderr=subprocess.DEVNULL)
    return gr, fa


def _run(exe, graph, fasta, k, b, m, a, mode, env, out):
    r = subprocess.run([exe, graph, fasta, str(k), str(b), str(m), str(a), mode, str(out)], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    ev = re.search(r"resolve-events: (.*)", r.stderr)
    assert ev, r.stderr[-500:]
    return {k_: int(v) for k_, v in (x.split("=") for x in ev.group(1).split())}


def _env(mode, nostats, sched, limit):
    # (emu_check has no 16-wavefront instantiation of the big variant with event counters: 4 wavefronts there - more than two, so the same path)
    env = {"EMU_NW": "16" if (nostats or mode.startswith("medium")) else "4", "EMU_LIMIT": str(limit), "EMU_FP_CHECK": "1"}
    if nostats:
        env["EMU_NOSTATS"] = "1"
    if sched:
        env["EMU_SCHED"] = sched
    return env


@pytest.mark.parametrize("sched", ["", "rr", "rev"])
@pytest.mark.parametrize("nostats", [False, True])
@pytest.mark.parametrize("mode", ["medium", "big"])
@pytest.mark.parametrize("name", ["inv_k25", "collinear6", "tandem4"])
def test_resolved_vote_on_goldens(emu_resolve, case_dir, name, mode, nostats, sched, tmp_path):
    from tests.conftest import Case
    c = Case(name, case_dir)
    ev = _run(emu_resolve, c.graph, c.fasta, c.k, c.b, c.m, c.a, mode, _env(mode, nostats, sched, 25), tmp_path / "emu")
    assert ev["resolved"] > 0
    if name != "inv_k25":                        # (k = 15: windows of several chunks, repeats that meet the path)
        assert ev["chunk1"] > 0 and ev["repeat_hit"] > 0


@pytest.mark.parametrize("mode,env", [("medium", {"EMU_SEG_CAP": "2000", "EMU_SEG_GAP": "777", "EMU_NW": "16", "EMU_NOSTATS": "1", "EMU_LIMIT": "80", "EMU_FP_CHECK": "1"}),
                                      ("big", {"EMU_SEG_CAP": "2000", "EMU_SEG_GAP": "100000", "EMU_NW": "16", "EMU_NOSTATS": "1", "EMU_LIMIT": "80", "EMU_SCHED": "rr", "EMU_FP_CHECK": "1"})])
def test_resolved_vote_with_segments(emu_resolve, case_dir, mode, env, tmp_path):
    """The SEG instantiations, with the knobs of tests/test_host_cpu.py (fewer seeds)."""
    from tests.conftest import Case
    c = Case("inv_k25", case_dir)
    ev = _run(emu_resolve, c.graph, c.fasta, c.k, c.b, c.m, c.a, mode, env, tmp_path / "emu")
    assert ev["resolved"] > 0


@pytest.mark.parametrize("nostats", [False, True])
@pytest.mark.parametrize("mode", ["medium", "big", "medium-runs", "big-runs"])
def test_resolved_vote_on_the_synthetic_input(emu_resolve, synth, mode, nostats, tmp_path):
    gr, fa = synth
    ev = _run(emu_resolve, gr, fa, 15, 200, 50, 150, mode, _env(mode, nostats, "rr" if mode.startswith("big") else "", 30), tmp_path / "emu")
    assert ev["resolved"] > 0 and ev["chunk1"] > 0 and ev["above_max"] > 0 and ev["items_full"] == 0
    if mode.endswith("-runs"):
        assert ev["used_beyond_64"] > 0 and ev["repeat_hit"] > 0 and ev["round2"] > 0, ev
