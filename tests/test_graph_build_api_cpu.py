"""CPU tests (no GPU) of the public surface of the graph build on the device: the C ABI and its ctypes binding know lcb_graph_build, the
layout of lcb_graph_build_stats is the header's, the ABI version stays 6, null or empty arguments are refused by name, the Python API
refuses an unknown option before anything is created, the CLI refuses an unknown LCB_JUNCTIONS before it loads anything, the file
route (LCB_JUNCTIONS=file or unset) still opens --graph, and without a HIP device the call says so. The parity tests are
tests/test_graph_emu.py (emulator) and tests/test_gpu_graph_build.py (MI355X)."""
import ctypes as C
import os
import subprocess

import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests.cli_inputs import cli as _cli, has_gpu as _has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_and_header_agree_on_the_new_surface(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    assert "lcb_graph_build" in api.EXPORTS and hasattr(lib, "lcb_graph_build")
    assert lib.lcb_abi_version() == 6 and api.ABI_VERSION == 6
    assert sibeliaz_amd.GraphBuildStats is api.GraphBuildStats and callable(sibeliaz_amd.JunctionStorage.build)
    fields = [f for f, _ in api.GraphBuildStats._fields_]
    assert fields[0] == "junctions" and {"raw_occurrences", "kept_occurrences", "vertices", "patched", "download_bytes", "peak_device_bytes", "parse_ms", "abundance_ms",
                                         "compact_ms", "download_ms", "csr_ms"} <= set(fields)
    # the prototype the binding assumes is the header's (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text('#include "lcb.h"\ntypedef lcb_graph* (*build_fn)(const char* const*, int, int, int, int, int, const lcb_junction_opts_ex*, lcb_graph_build_stats*);\n'
                     "build_fn the_call(void) { return lcb_graph_build; }\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    assert len(lib.lcb_graph_build.argtypes) == 8
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lcb.h"\n'
                   'int main(void) { printf("%zu %d %zu %zu", sizeof(lcb_graph_build_stats), LCB_ABI_VERSION, sizeof(lcb_junction_stats_ex), sizeof(lcb_junction_opts_ex));\n'
                   + "".join('printf(" %%zu", offsetof(lcb_graph_build_stats, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(api.GraphBuildStats), 6, C.sizeof(api.JunctionStatsEx), C.sizeof(api.JunctionOptsEx)] + [getattr(api.GraphBuildStats, f).offset for f in fields]
    assert got == want


def _call(lib, files, k=15, n=None, opts=None):
    arr = (C.c_char_p * max(1, len(files)))(*files) if files is not None else None
    st = api.GraphBuildStats()
    h = lib.lcb_graph_build(arr, len(files) if n is None else n, k, 150, 1, 0, opts, C.byref(st))
    return h, lib.lcb_last_error().decode()


def test_null_or_empty_arguments_fail_with_a_message_that_names_the_call(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTT\n")
    for files, n in ((None, 1), ([], 0), ([os.fsencode(str(fa))], 0), ([os.fsencode(str(fa))], -3)):
        arr = (C.c_char_p * max(1, len(files)))(*files) if files is not None else None
        assert not lib.lcb_graph_build(arr, n, 15, 150, 1, 0, None, None)
        assert "lcb_graph_build" in lib.lcb_last_error().decode()
    arr = (C.c_char_p * 2)(os.fsencode(str(fa)), None)
    assert not lib.lcb_graph_build(arr, 2, 15, 150, 1, 0, None, None)
    assert "lcb_graph_build" in lib.lcb_last_error().decode() and "null" in lib.lcb_last_error().decode()
    for k in (0, 16, 33, -1):
        h, msg = _call(lib, [os.fsencode(str(fa))], k=k)
        assert not h and "lcb_graph_build" in msg and str(k) in msg
    o = api.JunctionOptsEx()
    o.partitions = 65
    h, msg = _call(lib, [os.fsencode(str(fa))], opts=C.byref(o))
    assert not h and "partitions" in msg
    o = api.JunctionOptsEx()
    o.abi = 5
    h, msg = _call(lib, [os.fsencode(str(fa))], opts=C.byref(o))
    assert not h and "abi" in msg


def test_python_refuses_unknown_options_before_anything_is_created(built, tmp_path):
    missing = str(tmp_path / "does_not_exist.fa")          # reading it would be an LcbError, not a TypeError
    for name in ("table_bits", "tiles", "reserved", "abundances"):
        with pytest.raises(TypeError, match=name):
            sibeliaz_amd.JunctionStorage.build([missing], 15, **{name: 3})


@pytest.mark.parametrize("value", ["x", "Device", "gpu", "File", "host"])
def test_cli_rejects_an_unknown_junction_route_before_loading(built, tmp_path, value):
    out = tmp_path / "out"
    r = _cli(str(tmp_path / "no.bin"), str(tmp_path / "no.fa"), out, LCB_JUNCTIONS=value)
    assert r.returncode == 1
    assert r.stderr == "error: LCB_JUNCTIONS is '%s': it is file (the default) or device\n" % value
    assert r.stdout == "" and not out.exists()


def test_the_default_route_still_reads_the_junction_file(built, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTTACGATCGATCGGCTAGCTAGCATCGACT\n")
    runs = [_cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out"), _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_JUNCTIONS="file"),
            _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_JUNCTIONS="")]
    for r in runs:
        assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and r.stderr == "error: Can't read the input file\n"
    assert not (tmp_path / "out").exists()


def test_the_build_fails_loudly_without_a_gpu(built, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is present")
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTTACGATCGATCGGCTAGCTAGCATCGACT\n")
    with pytest.raises(sibeliaz_amd.LcbError, match="no HIP device available: lcb_graph_build runs only on the GPU"):
        sibeliaz_amd.JunctionStorage.build([str(fa)], 15)
    # ... and so does the CLI on the device route, where the file route fails on its missing --graph
    r = _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_JUNCTIONS="device")
    assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and "lcb_graph_build" in r.stderr and "no HIP device" in r.stderr
