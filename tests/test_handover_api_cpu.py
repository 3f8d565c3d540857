"""CPU tests (no GPU) of the public surface of the hand-over route: the C ABI and its ctypes binding know lcb_open_fasta, the layout of
lcb_open_stats is the header's, the ABI version stays 6, argument errors come with their message before any device is touched, an
unreadable FASTA gives the parser's text, without a HIP device the call says so and leaves both outputs NULL, and the CLI refuses every
bad LCB_HANDOVER value and combination before it loads anything while unset and `host` go on as before. The parity tests are
tests/test_handover_emu.py (emulator) and tests/test_gpu_handover.py (MI355X)."""
import ctypes as C
import os
import subprocess

import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests.cli_inputs import cli as _cli, has_gpu as _has_gpu, refused as _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_and_header_agree_on_the_new_surface(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    assert "lcb_open_fasta" in api.EXPORTS and hasattr(lib, "lcb_open_fasta")
    assert lib.lcb_abi_version() == 6 == api.ABI_VERSION
    assert sibeliaz_amd.OpenStats is api.OpenStats and sibeliaz_amd.open_fasta is api.open_fasta
    fields = [f for f, _ in api.OpenStats._fields_]
    assert fields == ["graph", "tables", "place_ms", "patch_ms", "csr_download_ms", "csr_download_bytes", "peak_device_bytes"]
    # the prototype the binding assumes is the header's (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text('#include "lcb.h"\ntypedef int (*open_fn)(const char* const*, int, int, int, int, const lcb_params*, int, const lcb_junction_opts_ex*, const lcb_device_opts*,\n'
                     "                       lcb_graph**, lcb_device**, lcb_open_stats*);\nopen_fn the_call(void) { return lcb_open_fasta; }\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    assert len(lib.lcb_open_fasta.argtypes) == 12
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lcb.h"\n'
                   'int main(void) { printf("%zu %d %zu %zu", sizeof(lcb_open_stats), LCB_ABI_VERSION, sizeof(lcb_graph_build_stats), sizeof(lcb_table_stats));\n'
                   + "".join('printf(" %%zu", offsetof(lcb_open_stats, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(api.OpenStats), 6, C.sizeof(api.GraphBuildStats), C.sizeof(api.TableStats)] + [getattr(api.OpenStats, f).offset for f in fields]
    assert got == want


def _call(lib, files, k=15, n=None, jopts=None, dopts=None, graph=True, device=True, params=True):
    arr = (C.c_char_p * max(1, len(files)))(*files) if files is not None else None
    g, d = C.c_void_p(0xdead), C.c_void_p(0xbeef)
    p = sibeliaz_amd.Params.make(k if 3 <= k <= 31 else 15)
    rc = lib.lcb_open_fasta(arr, len(files) if n is None else n, k, 150, 1, C.byref(p) if params else None, 0, jopts, dopts,
                            C.byref(g) if graph else None, C.byref(d) if device else None, None)
    return rc, lib.lcb_last_error().decode(), (g.value if graph else None), (d.value if device else None)


def test_argument_errors_come_with_their_message_and_before_any_device(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTT\n")
    one = [os.fsencode(str(fa))]
    for k in (16, 0, 2, 33, -1):                                     # even; outside 3..31
        rc, msg, g, d = _call(lib, one, k=k)
        assert rc != 0 and msg == "lcb_open_fasta: k must be odd and in 3..31, not %d" % k and g is None and d is None
    for files, n in ((None, 1), ([], 0), (one, 0), (one, -3)):
        rc, msg, g, d = _call(lib, files, n=n)
        assert rc != 0 and msg == "lcb_open_fasta: no FASTA file" and g is None and d is None
    for kw in (dict(graph=False), dict(device=False), dict(params=False)):
        rc, msg, g, d = _call(lib, one, **kw)
        assert rc != 0 and msg == "lcb_open_fasta: null argument" and not g and not d
    rc, msg, g, d = _call(lib, [os.fsencode(str(fa)), None], n=2)
    assert rc != 0 and msg == "lcb_open_fasta: FASTA path 1 is null"
    o = api.JunctionOptsEx()
    o.abi = 5
    rc, msg, g, d = _call(lib, one, jopts=C.byref(o))
    assert rc != 0 and msg == "lcb_junction_opts_ex.abi is 5, this library has LCB_ABI_VERSION 6" and g is None and d is None
    o = api.DeviceOpts()
    o.abi = 7
    rc, msg, g, d = _call(lib, one, dopts=C.byref(o))
    assert rc != 0 and msg == "lcb_device_opts.abi is 7, this library has LCB_ABI_VERSION 6" and g is None and d is None
    o = api.JunctionOptsEx()
    o.partitions = 65
    rc, msg, g, d = _call(lib, one, jopts=C.byref(o))
    assert rc != 0 and "partitions" in msg


def test_an_unreadable_fasta_gives_the_parsers_text(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTT\n")
    missing = str(tmp_path / "missing.fa")
    rc, msg, g, d = _call(lib, [os.fsencode(str(fa)), os.fsencode(missing)])
    assert rc != 0 and msg == "Can't open file " + missing and g is None and d is None
    with pytest.raises(sibeliaz_amd.LcbError, match="Can't open file"):
        sibeliaz_amd.open_fasta([missing], 15, sibeliaz_amd.Params.make(15))


def test_python_refuses_unknown_options_before_anything_is_created(built, tmp_path):
    missing = str(tmp_path / "does_not_exist.fa")          # reading it would be an LcbError, not a TypeError
    p = sibeliaz_amd.Params.make(15)
    for name in ("table_bits", "tiles", "reserved"):
        with pytest.raises(TypeError, match=name):
            sibeliaz_amd.open_fasta([missing], 15, p, **{name: 3})
    with pytest.raises(TypeError, match="seg_caps"):
        sibeliaz_amd.open_fasta([missing], 15, p, device_opts=dict(seg_caps=64))


def test_the_call_fails_loudly_without_a_gpu(built, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is present")
    lib = sibeliaz_amd.load_library()
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTTACGATCGATCGGCTAGCTAGCATCGACT\n")
    rc, msg, g, d = _call(lib, [os.fsencode(str(fa))])
    assert rc != 0 and msg.startswith("no HIP device available: lcb_open_fasta runs only on the GPU") and g is None and d is None
    with pytest.raises(sibeliaz_amd.LcbError, match="no HIP device available: lcb_open_fasta runs only on the GPU"):
        sibeliaz_amd.open_fasta([str(fa)], 15, sibeliaz_amd.Params.make(15))
    # ... and so does the CLI on the hand-over route
    r = _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_JUNCTIONS="device", LCB_HANDOVER="device")
    assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and "lcb_open_fasta" in r.stderr and "no HIP device" in r.stderr


@pytest.mark.parametrize("value", ["x", "Device", "gpu", "Host", "file", "hbm"])
def test_cli_rejects_an_unknown_handover_route_before_loading(built, tmp_path, value):
    _refused(tmp_path, "error: LCB_HANDOVER is '%s': it is host (the default) or device" % value, LCB_HANDOVER=value)
    _refused(tmp_path, "error: LCB_HANDOVER is '%s': it is host (the default) or device" % value, LCB_HANDOVER=value, LCB_JUNCTIONS="device")


def test_cli_rejects_the_combinations_the_route_does_not_support(built, tmp_path):
    needs = "error: LCB_HANDOVER=device requires LCB_JUNCTIONS=device: it is the graph built on the device that is handed over"
    _refused(tmp_path, needs, LCB_HANDOVER="device")
    _refused(tmp_path, needs, LCB_HANDOVER="device", LCB_JUNCTIONS="file")
    _refused(tmp_path, needs, LCB_HANDOVER="device", LCB_JUNCTIONS="", LCB_TABLES="device")
    _refused(tmp_path, "error: LCB_HANDOVER=device together with LCB_TABLES=host is not supported: the tables of a handed-over graph are built on the device (LCB_TABLES unset or device)",
             LCB_HANDOVER="device", LCB_JUNCTIONS="device", LCB_TABLES="host")
    for n in ("2", "8"):
        _refused(tmp_path, "error: LCB_HANDOVER=device together with LCB_GPUS=%s is not supported: the graph is handed over to the device of a single-GPU run (LCB_GPUS unset or 1)" % n,
                 LCB_HANDOVER="device", LCB_JUNCTIONS="device", LCB_GPUS=n)
    # the other switches' messages keep their text, and come first
    _refused(tmp_path, "error: LCB_SEEDS is 'x': it is host (the default) or device", LCB_HANDOVER="device", LCB_SEEDS="x")
    _refused(tmp_path, "error: LCB_TABLES is 'x': it is host (the default) or device", LCB_HANDOVER="device", LCB_TABLES="x")
    _refused(tmp_path, "error: LCB_JUNCTIONS is 'x': it is file (the default) or device", LCB_HANDOVER="device", LCB_JUNCTIONS="x")
    _refused(tmp_path, "error: LCB_TABLES=device together with LCB_GPUS=2 is not supported: the tables are built on the device of a single-GPU run (LCB_GPUS unset or 1)",
             LCB_HANDOVER="device", LCB_JUNCTIONS="device", LCB_TABLES="device", LCB_GPUS="2")


def test_unset_and_host_go_on_as_before(built, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTTACGATCGATCGGCTAGCTAGCATCGACT\n")
    runs = [_cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out"), _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_HANDOVER="host"),
            _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_HANDOVER=""), _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_HANDOVER="host", LCB_TABLES="host")]
    for r in runs:       # the file route reaches its junction file
        assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and r.stderr == "error: Can't read the input file\n"
    assert not (tmp_path / "out").exists()
    if not _has_gpu():   # ... and the device route its graph build, not the new call
        r = _cli(str(tmp_path / "no.bin"), str(fa), tmp_path / "out", LCB_HANDOVER="host", LCB_JUNCTIONS="device")
        assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and "lcb_graph_build" in r.stderr and "lcb_open_fasta" not in r.stderr
