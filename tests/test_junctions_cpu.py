"""The GPU junction finder's surface that needs no GPU: struct layouts of lcb_junction_opts / lcb_junction_stats, the argument
checks of lcb_junctions_build (made before the device is touched), and the loud failures of `build_junctions` and of
`lcb-mkgraph --gpu` on a machine without a GPU - there is no CPU fallback behind them, and no output file is left behind."""
import ctypes as C
import os
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


def test_junction_structs_have_the_layout_of_the_header(built, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lcb.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(lcb_junction_opts), '
                   'sizeof(lcb_junction_stats), offsetof(lcb_junction_opts, reserved), offsetof(lcb_junction_stats, write_ms)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(api.JunctionOpts), C.sizeof(api.JunctionStats), api.JunctionOpts.reserved.offset, api.JunctionStats.write_ms.offset]
    assert "lcb_junctions_build" in api.EXPORTS and hasattr(sibeliaz_amd.load_library(), "lcb_junctions_build")


@pytest.mark.parametrize("k", [24, 33])
def test_bad_k_is_refused_without_a_gpu(built, fasta, tmp_path, k):
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match="k must be odd"):
        sibeliaz_amd.build_junctions([fasta], k, out)
    _no_file(out)


def test_empty_file_list_is_refused(built, tmp_path):
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match="no FASTA file"):
        sibeliaz_amd.build_junctions([], 15, out)
    _no_file(out)


def test_missing_fasta_is_refused(built, fasta, tmp_path):
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match="cannot open"):
        sibeliaz_amd.build_junctions([fasta, str(tmp_path / "absent.fa")], 15, out)
    _no_file(out)


def test_other_abi_is_refused(built, fasta, tmp_path):
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match="LCB_ABI_VERSION"):
        sibeliaz_amd.build_junctions([fasta], 15, out, abi=5)
    _no_file(out)


def test_unknown_option_is_a_type_error(built, fasta, tmp_path):
    with pytest.raises(TypeError):
        sibeliaz_amd.build_junctions([fasta], 15, str(tmp_path / "g.bin"), bogus=1)


def test_build_junctions_fails_loudly_without_gpu(built, fasta, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is present")
    out = str(tmp_path / "g.bin")
    with pytest.raises(sibeliaz_amd.LcbError, match="no CPU fallback"):
        sibeliaz_amd.build_junctions([fasta], 15, out)
    _no_file(out)


def test_tool_gpu_flag_fails_loudly_without_gpu(built, fasta, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is present")
    out = str(tmp_path / "g.bin")
    env = {k: v for k, v in os.environ.items() if k != "LCB_LIB"}
    r = subprocess.run([MKGRAPH, "--gpu", "0", "-k", "15", "-o", out, fasta], capture_output=True, text=True, env=env)
    assert r.returncode == 1
    assert "lcb-mkgraph: error:" in r.stderr and "no CPU fallback" in r.stderr
    _no_file(out)


def test_tool_gpu_flag_with_missing_library(built, fasta, tmp_path):
    out = str(tmp_path / "g.bin")
    r = subprocess.run([MKGRAPH, "--gpu", "0", "-k", "15", "-o", out, fasta], capture_output=True, text=True, env=dict(os.environ, LCB_LIB="/nonexistent"))
    assert r.returncode == 1
    assert "lcb-mkgraph: error:" in r.stderr
    _no_file(out)


def test_tool_usage_names_the_new_flags_and_keeps_its_status(built):
    r = subprocess.run([MKGRAPH], capture_output=True, text=True)
    assert r.returncode == 2
    assert r.stderr.startswith("usage: lcb-mkgraph -k <odd 3..31> -o junctions.bin")
    for flag in ("--gpu", "--table-log2", "--tile-windows"):
        assert flag in r.stderr
