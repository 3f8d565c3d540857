"""GPU tests (-m gpu) of the table build on the device (csrc/tables.hip, lcb_table_kernels.h): a device created with tables="device" holds,
byte for byte, the tables a device created with tables="host" holds - on the goldens, on segmented device tables, on the synthetic
patterns of tests/table_inputs.py, on the edge inputs and on an input without a position - and is a device like any other: the same
per-seed results, the same seeds, the reference's blocks, through Python and through the CLI. Exact comparisons only.

Left out: a request that does not fit the free device memory. Without a field in lcb_device_opts (the ABI version stays) it can only be
reached by an input of tens of GB; the message is built by the same two lines as the seed enumeration's."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests import edge_inputs, table_inputs
from tests.test_gpu_parity import _setup
from tests.test_gpu_segments import _seg_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(api.TABLES)


def _same_tables(host, dev, what):
    assert host.tables == "host" and dev.tables == "device"
    for name in NAMES:
        a, b = host.read_table(name), dev.read_table(name)
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: table %s has shape %r on the host route, %r on the device route" % (what, name, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero(a != b)[0]
            raise AssertionError("%s: table %s differs first at element %d: host route %r, device route %r (%d of %d differ)" % (what, name, bad[0], a[bad[0]], b[bad[0]], len(bad), len(a)))
    hs, ds = host.table_stats, dev.table_stats
    assert hs["positions"] == ds["positions"] and hs["vertices"] == ds["vertices"]
    assert ds["sort_passes"] + ds["sort_passes_skipped"] == 4
    assert (hs["sort_passes"], hs["sort_passes_skipped"], hs["device_bytes"], hs["window_ms"], hs["csr_ms"], hs["sort_ms"], hs["gather_ms"]) == (0, 0, 0, 0, 0, 0, 0)
    if hs["positions"]:
        assert ds["upload_bytes"] < hs["upload_bytes"], "the device route uploads %d bytes, the host route %d" % (ds["upload_bytes"], hs["upload_bytes"])
        assert ds["device_bytes"] >= 16 * ds["positions"]


def _host_tables_match_the_graph(st, host):
    """The seam itself: what it reads back of the host route is the loaded graph."""
    assert host.read_table("pos_id").tobytes() == st.pos_id().tobytes() and host.read_table("pos_pos").tobytes() == st.pos_pos().tobytes()
    occ = host.read_table("occ_start")
    assert occ[0] == 0 and occ[-1] == st.n_positions() and (np.diff(occ.astype(np.int64)) >= 0).all()


def test_device_tables_equal_host_tables_on_goldens(built, case):
    st, p, host = _setup(case)
    dev = sibeliaz_amd.Device(st, p, 0, tables="device")
    _host_tables_match_the_graph(st, host)
    _same_tables(host, dev, case.name)
    rec = dev.read_table("occ_rec")
    assert (rec["id"] == st.pos_id()[_flat(st, dev, rec)]).all()


def _flat(st, dev, rec):
    """Host flat position of every occurrence record (one segment: g itself)."""
    assert (rec["cw"] >> 24 == 0).all()
    return rec["g"].astype(np.int64)


@pytest.mark.parametrize("flavour", ["many", "gap"])
def test_device_tables_equal_host_tables_on_segmented_tables(built, case, flavour):
    st, p, host = _seg_setup(case, flavour)
    st2, p2, dev = _seg_setup(case, flavour, tables="device")
    assert (host.read_table("seg_base") != 0).any(), "one segment only"
    _same_tables(host, dev, "%s, segments (%s)" % (case.name, flavour))


def test_device_tables_with_flat_indices_beyond_32_bits(built, case_dir):
    from tests.conftest import Case
    case = Case("twogenomes", case_dir)
    st, p, host = _seg_setup(case, "wide")
    st2, p2, dev = _seg_setup(case, "wide", tables="device")
    assert int(host.read_table("seg_base").max()) >= 1 << 32
    _same_tables(host, dev, "twogenomes, segments (wide)")


@pytest.mark.parametrize("n", table_inputs.SIZES)
@pytest.mark.parametrize("pattern", table_inputs.PATTERNS)
def test_device_tables_equal_host_tables_on_patterns(built, tmp_path, pattern, n):
    c = table_inputs.write(tmp_path, pattern, n)
    st = sibeliaz_amd.JunctionStorage(c["graph"], [c["fasta"]], c["k"], threads=2, abundance=c["a"])
    assert st.n_positions() == n and st.GetVerticesNumber() == c["vertices"]
    cs = st.chr_start()
    assert cs[c["empty_chr"] + 1] == cs[c["empty_chr"]], "the abundance filter did not empty chromosome %d" % c["empty_chr"]
    for b in table_inputs.MAX_BRANCH:
        p = sibeliaz_amd.Params.make(c["k"], b=b, m=50)
        host = sibeliaz_amd.Device(st, p, 0)
        dev = sibeliaz_amd.Device(st, p, 0, tables="device")
        _same_tables(host, dev, "%s, %d positions, max_branch %d" % (pattern, n, b))
        want = table_inputs.expected_passes(pattern, n)
        if want:
            assert (dev.table_stats["sort_passes"], dev.table_stats["sort_passes_skipped"]) == want
        if b == table_inputs.MAX_BRANCH[0]:
            win = dev.read_table("pos_win")
            assert int((win & 0xFFFF).max()) == b and int((win & 0xFFFF).min()) == 0, "the pattern no longer has a dense run and a sparse stretch"
    if pattern == "long_list" and n == table_inputs.SIZES[-1]:
        assert int(np.diff(dev.read_table("occ_start").astype(np.int64)).max()) > table_inputs.TILE
    # segments on a small input: the 64-bit instantiation of the build
    o = dict(seg_cap=1100, seg_gap=70001)
    _same_tables(sibeliaz_amd.Device(st, p, 0, **o), sibeliaz_amd.Device(st, p, 0, tables="device", **o), "%s, %d positions, segments" % (pattern, n))


@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_device_tables_equal_host_tables_on_edge_inputs(built, tmp_path, name):
    c = edge_inputs.build(name, str(tmp_path))
    st = sibeliaz_amd.JunctionStorage(c["graph"], c["fasta"], c["k"], threads=2, abundance=c["a"])
    p = sibeliaz_amd.Params.make(c["k"], b=c["b"], m=c["m"])
    host, dev = sibeliaz_amd.Device(st, p, 0), sibeliaz_amd.Device(st, p, 0, tables="device")
    _same_tables(host, dev, name)
    got, want = dev.enumerate_seeds(), st.seeds(2)
    assert got.tobytes() == want.tobytes()


def test_device_tables_of_an_input_without_positions(built, tmp_path):
    c = table_inputs.all_filtered(tmp_path)
    st = sibeliaz_amd.JunctionStorage(c["graph"], [c["fasta"]], c["k"], threads=1, abundance=c["a"])
    assert st.n_positions() == 0
    p = sibeliaz_amd.Params.make(c["k"], b=200, m=50)
    host, dev = sibeliaz_amd.Device(st, p, 0), sibeliaz_amd.Device(st, p, 0, tables="device")
    _same_tables(host, dev, "all filtered")
    assert dev.table_stats["positions"] == 0 and dev.table_stats["sort_passes"] == 0 and dev.table_stats["vertices"] > 0
    assert not dev.read_table("occ_start").any() and len(dev.read_table("occ_rec")) == 0
    # ... and the device is usable
    assert len(dev.enumerate_seeds()) == 0
    off, inst, score, _ = dev.process_seeds(np.zeros(0, dtype=sibeliaz_amd.SEED_DTYPE))
    assert len(off) == 1 and len(inst) == 0
    blocks = sibeliaz_amd.BlocksFinder(st, c["k"]).FindBlocks(50, 200, device=dev)
    assert len(blocks) == 0


def test_device_route_gives_a_device_like_any_other(built, case_dir):
    from tests.conftest import Case
    case = Case("smallb", case_dir)
    st, p, host = _setup(case)
    dev = sibeliaz_amd.Device(st, p, 0, tables="device")
    seeds = st.seeds(4)
    assert dev.enumerate_seeds().tobytes() == seeds.tobytes()
    a, b = host.process_seeds(seeds), dev.process_seeds(seeds)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    fa, fb = host.process_seeds_fp(seeds[:512]), dev.process_seeds_fp(seeds[:512])
    for x, y in zip(fa, fb):
        assert x.tobytes() == y.tobytes()
    dev.mark_used([[10, 200]])
    host.mark_used([[10, 200]])
    for x, y in zip(host.process_seeds(seeds[:512])[:3], dev.process_seeds(seeds[:512])[:3]):
        assert x.tobytes() == y.tobytes()
    dev.reset_used()
    blocks = sibeliaz_amd.BlocksFinder(st, case.k).FindBlocks(case.m, case.b, device=dev)
    text = "".join("%d\t%d\t%d\t%d\n" % (int(b["id"]), int(b["chr"]), int(b["start"]), int(b["end"])) for b in blocks)
    assert hashlib.sha256(text.encode()).hexdigest() == hashlib.sha256(case.golden("pretrim.tsv").encode()).hexdigest()


def test_table_read_checks_its_arguments(built, case_dir):
    from tests.conftest import Case
    case = Case("smallb", case_dir)
    st, p, dev = _setup(case, tables="device")
    n = st.n_positions()
    buf = np.zeros(8, dtype="<u4")
    for table, first, count, nbytes, words in ((99, 0, 8, 32, ("99",)), (api.TABLES["pos_win"][0], n - 4, 8, 32, (str(n - 4), str(n))), (api.TABLES["pos_win"][0], 0, 8, 31, ("31", "32"))):
        assert dev.L.lcb_device_table_read(dev.h, table, first, count, buf.ctypes.data, nbytes) != 0
        msg = dev.L.lcb_last_error().decode()
        assert "lcb_device_table_read" in msg and all(w in msg for w in words), msg
    # a range that crosses nothing, in the middle
    whole = dev.read_table("pos_win")
    assert dev.L.lcb_device_table_read(dev.h, api.TABLES["pos_win"][0], 100, 8, buf.ctypes.data, 32) == 0
    assert buf.tobytes() == whole[100:108].tobytes()


def test_cli_with_device_tables_writes_the_reference_file(built, case_dir, tmp_path):
    from tests.conftest import Case
    case = Case("smallb", case_dir)
    out = str(tmp_path / "cli")
    r = subprocess.run([os.path.join(ROOT, "sibeliaz_amd", "bin", "sibeliaz-lcb"), "--graph", case.graph, case.fasta, "-k", str(case.k), "-b", str(case.b),
                        "-o", out, "-m", str(case.m), "-t", "4", "--abundance", str(case.a), "--noseq"], capture_output=True, text=True,
                       env=dict(os.environ, LCB_TABLES="device", LCB_SEEDS="device", LCB_VERBOSE="1"))
    assert r.returncode == 0, r.stderr
    assert "lcb: device tables=device positions=" in r.stderr and "lcb: device seeds=" in r.stderr
    assert open(os.path.join(out, "blocks_coords.gff")).read() == case.golden("ref.gff")
