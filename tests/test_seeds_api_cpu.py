"""CPU tests (no GPU) of the public surface of the device seed enumeration: the C ABI and its ctypes binding know both entry points and
refuse a null device by name, the Python API refuses an unknown seeds= spelling, the CLI refuses an unknown LCB_SEEDS before it loads
anything, and the synthetic inputs of tests/seed_inputs.py have the properties the emulator and GPU tests rely on. The parity tests
are tests/test_seeds_emu.py (emulator) and tests/test_gpu_seeds.py (MI355X)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests import cli_inputs, seed_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_knows_the_new_entry_points(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    for name in ("lcb_device_enumerate_seeds", "lcb_device_sort_seeds", "lcb_gpus_device"):
        assert name in api.EXPORTS and hasattr(lib, name)
    assert lib.lcb_device_enumerate_seeds.restype is C.c_int64
    assert hasattr(sibeliaz_amd.Device, "enumerate_seeds") and hasattr(sibeliaz_amd.Device, "sort_seeds")
    # the ctypes mirror of lcb_seed_stats against the header compiled by gcc
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lcb.h"\nint main(void) { printf("%zu %zu %zu %d\\n", sizeof(lcb_seed_stats), '
                   'offsetof(lcb_seed_stats, device_bytes), offsetof(lcb_seed_stats, copy_ms), LCB_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(api.SeedStats), api.SeedStats.device_bytes.offset, api.SeedStats.copy_ms.offset, 6]


def test_null_arguments_fail_with_a_message_that_names_the_call(built):
    lib = sibeliaz_amd.load_library()
    out, st = C.c_void_p(), api.SeedStats()
    assert lib.lcb_device_enumerate_seeds(None, C.byref(out), C.byref(st)) == -1
    assert "lcb_device_enumerate_seeds" in lib.lcb_last_error().decode()
    seeds = np.zeros(3, dtype=sibeliaz_amd.SEED_DTYPE)
    assert lib.lcb_device_sort_seeds(None, seeds.ctypes.data, 3) != 0
    assert "lcb_device_sort_seeds" in lib.lcb_last_error().decode()
    assert lib.lcb_device_sort_seeds(None, seeds.ctypes.data, -1) != 0
    assert "lcb_device_sort_seeds" in lib.lcb_last_error().decode()
    assert not lib.lcb_gpus_device(None, 0)
    assert "lcb_gpus_device" in lib.lcb_last_error().decode()


def test_find_blocks_rejects_an_unknown_seeds_spelling(built, case):
    st = sibeliaz_amd.JunctionStorage(case.graph, [case.fasta], case.k, 2, case.a)
    finder = sibeliaz_amd.BlocksFinder(st, case.k)
    with pytest.raises(ValueError, match="seeds='gpu'"):
        finder.FindBlocks(case.m, case.b, seeds="gpu")


@pytest.mark.parametrize("value", ["bogus", "Device", "gpu"])
def test_cli_rejects_an_unknown_seed_route_before_loading(built, case, tmp_path, value):
    out = tmp_path / "out"
    r = cli_inputs.cli(case.graph, case.fasta, out, args=("-k", str(case.k), "-b", str(case.b), "-m", str(case.m), "-a", str(case.a)), LCB_SEEDS=value)
    assert r.returncode == 1
    assert r.stderr.startswith("error:") and "LCB_SEEDS" in r.stderr and value in r.stderr
    assert r.stdout == "" and not out.exists()


@pytest.mark.parametrize("params", seed_inputs.HEAVY, ids=lambda p: "heavy_%d_%d_%d_%d" % p)
def test_synthetic_inputs_have_the_properties_they_stand_for(built, tmp_path_factory, params):
    tmp = tmp_path_factory.mktemp("heavy")
    graph, fasta = seed_inputs.heavy(tmp, *params)
    st = sibeliaz_amd.JunctionStorage(graph, [fasta], seed_inputs.K, 2, seed_inputs.ABUNDANCE)
    seed_inputs.check_property(params, seed_inputs.ABUNDANCE, st.seeds(2))
    if params == seed_inputs.FILTERED[0]:
        st = sibeliaz_amd.JunctionStorage(graph, [fasta], seed_inputs.K, 2, seed_inputs.FILTERED[1])
        seed_inputs.check_property(params, seed_inputs.FILTERED[1], st.seeds(2))
