"""CPU tests (no GPU) of the public surface of the table build on the device: the C ABI and its ctypes binding know both entry points, the
layout of lcb_table_stats is the header's, the ABI version stays 6, a null graph or device is refused by name, the Python API refuses an
unknown tables= spelling before anything is created, the CLI refuses an unknown LCB_TABLES (and LCB_TABLES=device with several GPUs)
before it loads anything, and the synthetic inputs of tests/table_inputs.py have the properties the emulator and GPU tests rely on. The
parity tests are tests/test_tables_emu.py (emulator) and tests/test_gpu_tables.py (MI355X)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests import cli_inputs, table_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_and_header_agree_on_the_new_surface(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    for name in ("lcb_device_create_tables", "lcb_device_table_read"):
        assert name in api.EXPORTS and hasattr(lib, name)
    assert lib.lcb_abi_version() == 6 and api.ABI_VERSION == 6
    fields = [f for f, _ in api.TableStats._fields_]
    ids = ["LCB_TABLE_POS_ID", "LCB_TABLE_POS_POS", "LCB_TABLE_POS_WIN", "LCB_TABLE_POS_CH", "LCB_TABLE_POS_REV_CH", "LCB_TABLE_OCC_START", "LCB_TABLE_OCC_REC",
           "LCB_TABLE_CHR_LO_HI", "LCB_TABLE_SEG_BASE"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lcb.h"\nint main(void) { printf("%zu %d %d %d %zu", sizeof(lcb_table_stats), LCB_ABI_VERSION, LCB_TABLES_HOST, LCB_TABLES_DEVICE, sizeof(lcb_device_opts));\n'
                   + "".join('printf(" %%zu", offsetof(lcb_table_stats, %s));\n' % f for f in fields) + "".join('printf(" %%d", %s);\n' % i for i in ids) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(api.TableStats), 6, api.TABLE_ROUTES["host"], api.TABLE_ROUTES["device"], C.sizeof(api.DeviceOpts)] + [getattr(api.TableStats, f).offset for f in fields]
    want += [api.TABLES[n][0] for n in ("pos_id", "pos_pos", "pos_win", "pos_ch", "pos_rev_ch", "occ_start", "occ_rec", "chr_lo_hi", "seg_base")]
    assert got == want
    assert api.OCC_REC_DTYPE.itemsize == 16 and api.TABLES["chr_lo_hi"][1].itemsize == 8


def test_null_arguments_fail_with_a_message_that_names_the_call(built):
    lib = sibeliaz_amd.load_library()
    st, p = api.TableStats(), sibeliaz_amd.Params.make(15)
    for route in (0, 1):
        assert not lib.lcb_device_create_tables(None, C.byref(p), 0, None, route, C.byref(st))
        assert "lcb_device_create_tables" in lib.lcb_last_error().decode()
    buf = np.zeros(4, dtype="<u4")
    assert lib.lcb_device_table_read(None, 0, 0, 4, buf.ctypes.data, 16) != 0
    assert "lcb_device_table_read" in lib.lcb_last_error().decode()


def test_python_refuses_an_unknown_tables_spelling_before_anything_is_created(built):
    class Untouchable:          # any use of the storage would be an AttributeError, not an LcbError
        pass
    for spelling in ("gpu", "Device", "", None, 1):
        with pytest.raises(sibeliaz_amd.LcbError, match="tables="):
            sibeliaz_amd.Device(Untouchable(), sibeliaz_amd.Params.make(15), 0, tables=spelling)


def test_python_refuses_an_unknown_device_option_wherever_one_is_taken(built):
    class Untouchable:          # any use of the storage would be an AttributeError, not a TypeError
        pass
    p = sibeliaz_amd.Params.make(15)
    for make in (lambda: sibeliaz_amd.Device(Untouchable(), p, 0, seg_caps=64), lambda: sibeliaz_amd.GpuSet(Untouchable(), p, [0], seg_caps=64),
                 lambda: sibeliaz_amd.BlocksFinder(Untouchable(), 15).FindBlocksGpus(50, 200, [0], device_opts=dict(seg_caps=64))):
        with pytest.raises(TypeError, match="unknown device option 'seg_caps'"):
            make()


def _cli(case, out, **env):
    return cli_inputs.cli(case.graph, case.fasta, out, args=("-k", str(case.k), "-b", str(case.b), "-m", str(case.m), "-a", str(case.a)), **env)


@pytest.mark.parametrize("value", ["x", "Device", "gpu"])
def test_cli_rejects_an_unknown_table_route_before_loading(built, case, tmp_path, value):
    out = tmp_path / "out"
    r = _cli(case, out, LCB_TABLES=value)
    assert r.returncode == 1
    assert r.stderr.startswith("error:") and "LCB_TABLES" in r.stderr and value in r.stderr
    assert r.stdout == "" and not out.exists()


def test_cli_rejects_device_tables_on_several_gpus_naming_both(built, case, tmp_path):
    out = tmp_path / "out"
    r = _cli(case, out, LCB_TABLES="device", LCB_GPUS="2")
    assert r.returncode == 1
    assert r.stderr.startswith("error:") and "LCB_TABLES" in r.stderr and "LCB_GPUS" in r.stderr
    assert r.stdout == "" and not out.exists()


@pytest.mark.parametrize("pattern", table_inputs.PATTERNS)
def test_synthetic_inputs_load_and_have_the_properties_they_stand_for(built, tmp_path, pattern):
    for n in table_inputs.SIZES:
        c = table_inputs.write(tmp_path, pattern, n)
        st = sibeliaz_amd.JunctionStorage(c["graph"], [c["fasta"]], c["k"], 2, c["a"])
        assert st.n_positions() == n and st.GetVerticesNumber() == c["vertices"] <= table_inputs.MAX_ID + 1 and st.GetChrNumber() == c["chromosomes"]
        cs = np.asarray(st.chr_start())
        sizes = np.diff(cs.astype(np.int64))
        assert sizes[c["empty_chr"]] == 0 and (np.delete(sizes, c["empty_chr"]) > 0).all() and (sizes == 1).sum() >= 2
        vid, pos = np.asarray(st.pos_id()), np.asarray(st.pos_pos()).astype(np.int64)
        assert (vid == table_inputs.ids(pattern, n)).all()
        inner = np.ones(n, dtype=bool)
        inner[cs[1:-1][cs[1:-1] < n]] = False              # (the first position of a chromosome has no gap in front of it)
        gaps = np.diff(pos)[inner[1:]]
        assert (gaps == 1).sum() > 30 and (gaps == 1000).sum() >= 3
        counts = np.bincount(np.abs(vid))
        if pattern == "one_vertex":
            assert counts.max() == n
        elif pattern == "distinct":
            assert counts.max() == 1
        elif pattern == "both_signs":
            assert (vid < 0).any() and (vid > 0).any() and len(set(np.abs(vid[vid < 0])) & set(vid[vid > 0])) > 0
        elif pattern == "high_byte":
            assert len(set((np.abs(vid) >> 16) & 255)) > 1 and len(set(np.abs(vid) & 0xFFFF)) == 1
        elif pattern == "long_list" and n == table_inputs.SIZES[-1]:
            assert counts.max() > table_inputs.TILE


def test_input_without_positions_loads(built, tmp_path):
    c = table_inputs.all_filtered(tmp_path)
    st = sibeliaz_amd.JunctionStorage(c["graph"], [c["fasta"]], c["k"], 1, c["a"])
    assert st.n_positions() == 0 and st.GetChrNumber() == 2 and st.GetVerticesNumber() == 10
