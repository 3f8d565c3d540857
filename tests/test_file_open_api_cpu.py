"""CPU tests (no GPU) of the public surface of the junction file opened on the GPU: the C ABI and its ctypes binding know
lcb_graph_load_device and lcb_open_junctions with the header's prototypes, the ABI version stays 6, argument errors come with their
message before any device is touched, without a HIP device both calls say so and leave their outputs NULL, and the CLI refuses every
bad LCB_LOAD value and combination before it loads anything while unset, empty and `host` go on as before. The parity tests are
tests/test_file_emu.py (emulator) and tests/test_gpu_file_open.py (MI355X)."""
import ctypes as C
import os
import subprocess

import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests import file_inputs
from tests.cli_inputs import cli as _cli, has_gpu as _has_gpu, refused as _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_and_header_agree_on_the_new_surface(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    for name in ("lcb_graph_load_device", "lcb_open_junctions"):
        assert name in api.EXPORTS and hasattr(lib, name)
    assert lib.lcb_abi_version() == 6 == api.ABI_VERSION
    assert sibeliaz_amd.open_junctions is api.open_junctions and callable(sibeliaz_amd.JunctionStorage.load_device)
    # the prototypes the binding assumes are the header's (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text('#include "lcb.h"\n'
                     "typedef lcb_graph* (*load_fn)(const char*, const char* const*, int, int, int, int, int, const lcb_junction_opts_ex*, lcb_graph_build_stats*);\n"
                     "typedef int (*open_fn)(const char*, const char* const*, int, int, int, int, const lcb_params*, int, const lcb_junction_opts_ex*, const lcb_device_opts*,\n"
                     "                       lcb_graph**, lcb_device**, lcb_open_stats*);\n"
                     "load_fn the_load(void) { return lcb_graph_load_device; }\nopen_fn the_open(void) { return lcb_open_junctions; }\n"
                     "int the_abi(void) { return LCB_ABI_VERSION; }\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    assert len(lib.lcb_graph_load_device.argtypes) == 9 and lib.lcb_graph_load_device.restype is C.c_void_p
    assert len(lib.lcb_open_junctions.argtypes) == 13
    assert lib.lcb_graph_load_device.argtypes[1:] == lib.lcb_graph_build.argtypes and lib.lcb_open_junctions.argtypes[1:] == lib.lcb_open_fasta.argtypes


def _inputs(tmp_path):
    c = file_inputs.build("signed_ids", tmp_path)
    return os.fsencode(c["graph"]), [os.fsencode(f) for f in c["fasta"]], c


def _load(lib, graph, files, k=15, n=None, opts=None):
    arr = (C.c_char_p * max(1, len(files)))(*files) if files is not None else None
    h = lib.lcb_graph_load_device(graph, arr, len(files) if n is None else n, k, 150, 1, 0, opts, None)
    return h, lib.lcb_last_error().decode()


def _open(lib, graph, files, k=15, n=None, jopts=None, dopts=None, out_graph=True, out_device=True, params=True):
    arr = (C.c_char_p * max(1, len(files)))(*files) if files is not None else None
    g, d = C.c_void_p(0xdead), C.c_void_p(0xbeef)
    p = sibeliaz_amd.Params.make(15)
    rc = lib.lcb_open_junctions(graph, arr, len(files) if n is None else n, k, 150, 1, C.byref(p) if params else None, 0, jopts, dopts,
                                C.byref(g) if out_graph else None, C.byref(d) if out_device else None, None)
    return rc, lib.lcb_last_error().decode(), (g.value if out_graph else None), (d.value if out_device else None)


def test_argument_errors_come_with_their_message_and_before_any_device(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    graph, files, _ = _inputs(tmp_path)
    for k in (16, 0, -1):                                            # the loader's own check and words
        h, msg = _load(lib, graph, files, k=k)
        assert not h and msg == "value of K must be odd"
        rc, msg, g, d = _open(lib, graph, files, k=k)
        assert rc != 0 and msg == "value of K must be odd" and g is None and d is None
    for gr, fl, n in ((None, files, None), (graph, None, 1), (graph, files, 0), (graph, files, -2)):
        h, msg = _load(lib, gr, fl, n=n)
        assert not h and msg == "lcb_graph_load_device: missing input files"
        rc, msg, g, d = _open(lib, gr, fl, n=n)
        assert rc != 0 and msg == "lcb_open_junctions: missing input files" and g is None and d is None
    for kw in (dict(out_graph=False), dict(out_device=False), dict(params=False)):
        rc, msg, g, d = _open(lib, graph, files, **kw)
        assert rc != 0 and msg == "lcb_open_junctions: null argument" and not g and not d
    h, msg = _load(lib, graph, files + [None], n=2)
    assert not h and msg == "lcb_graph_load_device: FASTA path 1 is null"
    o = api.JunctionOptsEx()
    o.abi = 5
    h, msg = _load(lib, graph, files, opts=C.byref(o))
    assert not h and msg == "lcb_junction_opts_ex.abi is 5, this library has LCB_ABI_VERSION 6"
    rc, msg, g, d = _open(lib, graph, files, jopts=C.byref(o))
    assert rc != 0 and msg == "lcb_junction_opts_ex.abi is 5, this library has LCB_ABI_VERSION 6" and g is None and d is None
    o = api.DeviceOpts()
    o.abi = 7
    rc, msg, g, d = _open(lib, graph, files, dopts=C.byref(o))
    assert rc != 0 and msg == "lcb_device_opts.abi is 7, this library has LCB_ABI_VERSION 6" and g is None and d is None
    # files that cannot be read give the loader's and the parser's texts
    missing = os.fsencode(str(tmp_path / "missing"))
    h, msg = _load(lib, missing, files)
    assert not h and msg == "Can't read the input file"
    rc, msg, g, d = _open(lib, graph, [missing])
    assert rc != 0 and msg == "Can't open file " + os.fsdecode(missing) and g is None and d is None


def test_python_refuses_unknown_options_before_anything_is_created(built, tmp_path):
    missing = str(tmp_path / "does_not_exist")             # reading it would be an LcbError, not a TypeError
    p = sibeliaz_amd.Params.make(15)
    for name in ("table_log2", "partitions", "tiles"):     # (the junction finder's knobs mean nothing here)
        with pytest.raises(TypeError, match=name):
            sibeliaz_amd.open_junctions(missing, [missing], 15, p, **{name: 3})
        with pytest.raises(TypeError, match=name):
            sibeliaz_amd.JunctionStorage.load_device(missing, [missing], 15, **{name: 3})
    with pytest.raises(TypeError, match="seg_caps"):
        sibeliaz_amd.open_junctions(missing, [missing], 15, p, device_opts=dict(seg_caps=64))


def test_both_calls_fail_loudly_without_a_gpu(built, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is present")
    lib = sibeliaz_amd.load_library()
    graph, files, c = _inputs(tmp_path)
    h, msg = _load(lib, graph, files)
    assert not h and msg.startswith("no HIP device available: lcb_graph_load_device runs only on the GPU") and "lcb_graph_load" in msg.split("fallback")[1]
    rc, msg, g, d = _open(lib, graph, files)
    assert rc != 0 and msg.startswith("no HIP device available: lcb_open_junctions runs only on the GPU") and g is None and d is None
    with pytest.raises(sibeliaz_amd.LcbError, match="no HIP device available: lcb_graph_load_device runs only on the GPU"):
        sibeliaz_amd.JunctionStorage.load_device(c["graph"], c["fasta"], 15)
    with pytest.raises(sibeliaz_amd.LcbError, match="no HIP device available: lcb_open_junctions runs only on the GPU"):
        sibeliaz_amd.open_junctions(c["graph"], c["fasta"], 15, sibeliaz_amd.Params.make(15))
    # ... and so does the CLI with LCB_LOAD=device, with either seed route
    for seeds in ("host", "device"):
        r = _cli(c["graph"], c["fasta"][0], tmp_path / "out", LCB_LOAD="device", LCB_SEEDS=seeds)
        assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and "lcb_open_junctions" in r.stderr and "no HIP device" in r.stderr


@pytest.mark.parametrize("value", ["x", "Device", "gpu", "Host", "file", "hbm"])
def test_cli_rejects_an_unknown_load_route_before_loading(built, tmp_path, value):
    _refused(tmp_path, "error: LCB_LOAD is '%s': it is host (the default) or device" % value, LCB_LOAD=value)
    _refused(tmp_path, "error: LCB_LOAD is '%s': it is host (the default) or device" % value, LCB_LOAD=value, LCB_TABLES="device")


def test_cli_rejects_the_combinations_the_route_does_not_support(built, tmp_path):
    _refused(tmp_path, "error: LCB_LOAD=device together with LCB_JUNCTIONS=device is not supported: there is no file to load (the junctions come from the FASTA files)",
             LCB_LOAD="device", LCB_JUNCTIONS="device")
    _refused(tmp_path, "error: LCB_LOAD=device together with LCB_TABLES=host is not supported: the tables of a graph opened on the device are built there (LCB_TABLES unset or device)",
             LCB_LOAD="device", LCB_TABLES="host")
    for n in ("2", "8"):
        _refused(tmp_path, "error: LCB_LOAD=device together with LCB_GPUS=%s is not supported: the file is opened on the device of a single-GPU run (LCB_GPUS unset or 1)" % n,
                 LCB_LOAD="device", LCB_GPUS=n)
    # the other switches' messages keep their text, and come first
    _refused(tmp_path, "error: LCB_SEEDS is 'x': it is host (the default) or device", LCB_LOAD="device", LCB_SEEDS="x")
    _refused(tmp_path, "error: LCB_TABLES is 'x': it is host (the default) or device", LCB_LOAD="device", LCB_TABLES="x")
    _refused(tmp_path, "error: LCB_JUNCTIONS is 'x': it is file (the default) or device", LCB_LOAD="device", LCB_JUNCTIONS="x")
    _refused(tmp_path, "error: LCB_HANDOVER is 'x': it is host (the default) or device", LCB_LOAD="device", LCB_HANDOVER="x")
    _refused(tmp_path, "error: LCB_TABLES=device together with LCB_GPUS=2 is not supported: the tables are built on the device of a single-GPU run (LCB_GPUS unset or 1)",
             LCB_LOAD="device", LCB_TABLES="device", LCB_GPUS="2")
    # LCB_HANDOVER=device keeps requiring LCB_JUNCTIONS=device
    _refused(tmp_path, "error: LCB_HANDOVER=device requires LCB_JUNCTIONS=device: it is the graph built on the device that is handed over", LCB_LOAD="device", LCB_HANDOVER="device")


def test_unset_empty_and_host_go_on_as_before(built, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTAAACCCGGGTTTACGATCGATCGGCTAGCTAGCATCGACT\n")
    no = str(tmp_path / "no.bin")
    runs = [_cli(no, str(fa), tmp_path / "out"), _cli(no, str(fa), tmp_path / "out", LCB_LOAD="host"), _cli(no, str(fa), tmp_path / "out", LCB_LOAD=""),
            _cli(no, str(fa), tmp_path / "out", LCB_LOAD="host", LCB_TABLES="host"), _cli(no, str(fa), tmp_path / "out", LCB_LOAD="host", LCB_GPUS="2")]
    for r in runs:       # the host route reaches its junction file through lcb_graph_load
        assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and r.stderr == "error: Can't read the input file\n"
    assert not (tmp_path / "out").exists()
    # a refused file gives the loader's text on the host route, whatever LCB_LOAD says as long as it says host
    c = file_inputs.build("err_unordered", tmp_path)
    for env in ({}, {"LCB_LOAD": "host"}, {"LCB_LOAD": ""}):
        r = _cli(c["graph"], c["fasta"][0], tmp_path / "out", **env)
        assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and r.stderr == "error: " + c["error"] + "\n"
    if not _has_gpu():   # ... and LCB_LOAD=host with the junctions from the device is the graph build, not the new call
        r = _cli(no, str(fa), tmp_path / "out", LCB_LOAD="host", LCB_JUNCTIONS="device")
        assert r.returncode == 1 and r.stdout == "Loading the graph...\n" and "lcb_graph_build" in r.stderr and "lcb_open_junctions" not in r.stderr
