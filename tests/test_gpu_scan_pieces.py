"""GPU tests (-m gpu) of the one-workgroup scans of the device-building routes beyond their first piece (seedScan32 / seedScan64 of
lcb_seed_kernels.h, tableScan32/64 of lcb_table_kernels.h, graphScan of lcb_graph_kernels.h, junctionScan of lcb_junction_kernels.h):
every route that ends in one of them runs on the two inputs of tests/scan_inputs.py, on which each scan takes three pieces or more
(tests/test_scan_inputs_cpu.py asserts that against the host route), and gives what the host route gives.

  * lcb_device_sort_seeds on generated keys of 16, 17, 34 and 101 tiles (1, 2, 3 and 7 pieces of seedScan32), the six patterns of
    tests/test_gpu_seeds.py and one whose tile histograms are mostly 0 with a few entries of 1024;
  * the tables built on the device against the tables built on the host, flat (32-bit) and in segments with a gap (64-bit);
  * the seeds enumerated on both devices against the host enumerator, and the sort of that array shuffled;
  * the junction file opened on the device (JunctionStorage.load_device, open_junctions) against the host loader's graph and the
    HOST-route device's tables, in one tile and in tiles of 100003 records;
  * the junction finder (build_junctions, JunctionStorage.build, open_fasta) against the CPU lcb-mkgraph's file byte for byte, in one
    tile of 2735 blocks and in three tiles of 300000 windows.

Exact comparisons only. No FindBlocks on the packed file: its ids are not a genome's, and the engine is not what this tests."""
import os

import numpy as np
import pytest

import sibeliaz_amd
from tests import scan_inputs, seed_inputs
from tests.test_gpu_file_open import _describe, _graph_of
from tests.test_gpu_handover import _check as _check_open_fasta
from tests.test_gpu_handover import _mkgraph
from tests.test_gpu_seeds import TILE, _host_order, _keys, _same
from tests.test_gpu_tables import _same_tables

pytestmark = pytest.mark.gpu

PATTERNS = ["random", "count_top", "chr_only", "rank_low", "rank_wrap", "count_equal", "two_values"]
SORT_SIZES = [16 * TILE, 16 * TILE + 1, 33 * TILE + 17, 100 * TILE + 5]
LAYOUTS = {"flat": {}, "segments": dict(seg_cap=400000, seg_gap=70001)}


# ---- lcb_device_sort_seeds past one piece of seedScan32

@pytest.fixture(scope="module")
def sort_device(built, tmp_path_factory):
    graph, fasta = seed_inputs.no_seed(tmp_path_factory.mktemp("scan_sort"))
    st = sibeliaz_amd.JunctionStorage(graph, [fasta], seed_inputs.K, threads=1, abundance=seed_inputs.ABUNDANCE)
    dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(seed_inputs.K, b=200, m=50), 0)
    yield dev
    dev.close()
    st.close()


def _two_values(n):
    """The keys differ in byte 1 of the rank alone, which takes two values in alternating runs of three tiles: one pass, and of the 256
    histogram entries of a tile at most two are not 0 - 1024 for most tiles."""
    s = _keys(n, "two_values")                     # (no pattern of _keys: every key the same)
    assert len(np.unique(s["rank"])) <= 1
    s["rank"] = np.where((np.arange(n) // (3 * TILE)) % 2 == 0, 0x9A00, 0x1300).astype(np.uint64) | np.uint64(0x55)
    return s


@pytest.mark.parametrize("pattern", PATTERNS)
def test_device_sort_orders_generated_keys_past_one_piece(sort_device, pattern):
    for n in SORT_SIZES:
        s = _two_values(n) if pattern == "two_values" else _keys(n, pattern)
        before = s.copy()
        got = sort_device.sort_seeds(s)
        assert s.tobytes() == before.tobytes(), "sort_seeds changed its argument"
        want = _host_order(s)
        assert want.tobytes() != s.tobytes(), "%s, n = %d: the keys are in order already" % (pattern, n)
        assert got.tobytes() == want.tobytes(), "%s, n = %d" % (pattern, n)


# ---- the packed file: tables, seeds, the file route

@pytest.fixture(scope="module")
def packed(built, tmp_path_factory):
    """The input, the host loader's storage, the host enumerator's seeds and the description of the storage and a HOST-route device."""
    c = scan_inputs.packed(tmp_path_factory.mktemp("scan_packed"))
    st = sibeliaz_amd.JunctionStorage(c["graph"], c["fasta"], c["k"], threads=4, abundance=c["a"])
    assert st.n_positions() == c["kept"] and st.GetVerticesNumber() == c["vertices"]
    p = sibeliaz_amd.Params.make(c["k"], b=200, m=50)
    host = sibeliaz_amd.Device(st, p, 0, tables="host")
    want = _describe(st, host)
    host.close()
    yield dict(c=c, st=st, params=p, seeds=st.seeds(4), want=want)
    st.close()


@pytest.fixture(scope="module", params=sorted(LAYOUTS))
def devices(request, packed):
    opts = LAYOUTS[request.param]
    host = sibeliaz_amd.Device(packed["st"], packed["params"], 0, tables="host", **opts)
    dev = sibeliaz_amd.Device(packed["st"], packed["params"], 0, tables="device", **opts)
    yield request.param, host, dev
    dev.close()
    host.close()


def test_device_tables_equal_host_tables_on_the_packed_file(packed, devices):
    layout, host, dev = devices
    st = packed["st"]
    _same_tables(host, dev, "packed, " + layout)
    occ = dev.read_table("occ_start")
    assert int(occ[-1]) == st.n_positions() and len(occ) == st.GetVerticesNumber() + 1 > 4096 * 16
    assert (len(np.unique(host.read_table("seg_base"))) > 1) == (layout == "segments")          # segments: the 64-bit instantiations
    assert dev.table_stats["sort_passes"] >= 3                               # ids beyond 2^16: three digits tell keys apart


def test_device_seeds_equal_host_seeds_on_the_packed_file(packed, devices):
    layout, host, dev = devices
    want = packed["seeds"]
    assert len(want) > 3 * 16384
    _same(host.enumerate_seeds(), want, "packed, %s, host tables" % layout)
    got, stats = dev.enumerate_seeds(stats=True)
    _same(got, want, "packed, %s, device tables" % layout)
    assert stats["seeds"] == len(want) and stats["vertices"] == packed["st"].GetVerticesNumber() > 3 * 32768
    shuffled = want[np.random.default_rng(5).permutation(len(want))]
    assert shuffled.tobytes() != want.tobytes()
    assert dev.sort_seeds(shuffled).tobytes() == want.tobytes()


@pytest.mark.parametrize("tile", [None, 100003], ids=["one_tile", "tile100003"])
def test_file_opened_on_the_device_equals_the_loader_on_the_packed_file(packed, tile):
    c, yst, want = packed["c"], packed["st"], packed["want"]
    jopts = dict(tile_windows=tile) if tile else {}
    records = os.path.getsize(c["graph"]) // 12
    lst, lstats = sibeliaz_amd.JunctionStorage.load_device(c["graph"], c["fasta"], c["k"], abundance=c["a"], threads=4, stats=True, **jopts)
    got = _graph_of(lst)
    for key in got:
        assert got[key] == want[key], "packed: %s differs between lcb_graph_load_device and lcb_graph_load" % key
    lst.close()
    st, dev, stats = sibeliaz_amd.open_junctions(c["graph"], c["fasta"], c["k"], packed["params"], abundance=c["a"], threads=4, stats=True, **jopts)
    got = _describe(st, dev)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], "packed: %s differs between lcb_open_junctions and the host route" % key
    for s in (lstats, stats):
        assert s["raw_occurrences"] == scan_inputs.N and s["kept_occurrences"] == yst.n_positions()
        assert s["vertices"] == yst.GetVerticesNumber() and s["records"] == yst.GetChrNumber()
        assert s["tiles"] == ((records + tile - 1) // tile if tile else 1)
        assert s["patched"] == c["patched"]
    dev.close()
    st.close()


# ---- the junction finder with more than one block per lane of junctionScan

@pytest.fixture(scope="module")
def copies(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_copies")
    c = scan_inputs.fasta(tmp)
    c["graph"] = _mkgraph(c["fasta"], c["k"], str(tmp / "cpu.bin"))
    c["tmp"] = tmp
    return c


@pytest.mark.parametrize("tile,tiles", [(None, 1), (300000, 3)], ids=["one_tile", "tile300000"])
def test_junction_finder_writes_the_cpu_tools_file(copies, tile, tiles):
    out = str(copies["tmp"] / ("gpu_%s.bin" % tile))
    stats = sibeliaz_amd.build_junctions(copies["fasta"], copies["k"], out, **(dict(tile_windows=tile) if tile else {}))
    assert stats["tiles"] == tiles and stats["windows"] == copies["windows"] and stats["records"] == 1
    want = open(copies["graph"], "rb").read()
    assert len(want) == 12 * (stats["occurrences"] + 1) > 12 * 256
    assert open(out, "rb").read() == want


def test_graph_and_device_built_from_the_fasta_equal_the_two_steps(copies):
    k, a = copies["k"], 150
    st, dev, stats, yst = _check_open_fasta(copies["graph"], copies["fasta"], k, a, "copies")        # (against a host-route device)
    assert stats["tiles"] == 1 and yst.n_positions() > 256
    want = _graph_of(yst)
    dev.close()
    st.close()
    bst, bstats = sibeliaz_amd.JunctionStorage.build(copies["fasta"], k, abundance=a, threads=2, stats=True)
    got = _graph_of(bst)
    for key in want:
        assert got[key] == want[key], "copies: %s differs between lcb_graph_build and the two steps" % key
    assert bstats["tiles"] == 1
    bst.close()
