"""GPU tests (-m gpu) of the junction file opened on the device (lcb_graph_load_device, lcb_open_junctions, JunctionStorage.load_device,
sibeliaz_amd.open_junctions, LCB_LOAD=device; csrc/junctions.hip, lcb_file_kernels.h): the storage is the one JunctionStorage reads from
the same file on host threads, the device's nine tables are those of Device(that storage, params, tables="device") with the same device
options - on the committed goldens (whose files carry the reference's ids), the edge inputs, the heavy inputs and every legal
hand-packed file of tests/file_inputs.py; whatever the tile size; under segmented layouts with and without a gap; with the patched
letters in both copies; through FindBlocks and the CLI; with the loader's texts for the five defects and nothing left behind. Exact
comparisons only."""
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests import edge_inputs, file_inputs, seed_inputs
from tests.conftest import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sibeliaz_amd", "bin", "sibeliaz-lcb")
TABLE_NAMES = sorted(api.TABLES)


def _graph_of(st):
    n = st.GetChrNumber()
    return {"chromosomes": n, "names": [st.GetChrDescription(c) for c in range(n)], "lengths": [st.chr_len(c) for c in range(n)], "vertices": st.GetVerticesNumber(),
            "chr_start": st.chr_start().tobytes(), "pos_id": st.pos_id().tobytes(), "pos_pos": st.pos_pos().tobytes(), "seeds": st.seeds(2).tobytes()}


def _describe(st, dev):
    """Everything "the same graph and the same device" compares, as a dict of bytes / values (the host enumerator's seeds are made of
    posCh, posRevCh and the host CSR)."""
    out = _graph_of(st)
    for name in TABLE_NAMES:
        t = dev.read_table(name)
        out["table " + name] = (str(t.dtype), t.shape, t.tobytes())
    return out


_yard = {}


def _yardstick(graph, fasta, k, a, b, m, dopts):
    """The composed route: the loader's storage, and the description of it and of a device whose tables are built on the GPU from it
    with the same options; computed once per input and layout and left unchanged."""
    key = (graph, tuple(fasta), k, a, b, m, tuple(sorted(dopts.items())))
    if key not in _yard:
        skey = (graph, tuple(fasta), k, a)
        if skey not in _yard:
            _yard[skey] = sibeliaz_amd.JunctionStorage(graph, list(fasta), k, threads=2, abundance=a)
        st = _yard[skey]
        dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(k, b=b, m=m), 0, tables="device", **dopts)
        _yard[key] = (st, _describe(st, dev))
        dev.close()
    return _yard[key]


def _check(graph, fasta, k, a, what, b=200, m=50, dopts=None, **jopts):
    """load_device and open_junctions against the yardstick -> (storage, device, stats, the yardstick's storage); the caller closes
    device, then storage."""
    dopts = dopts or {}
    yst, want = _yardstick(graph, fasta, k, a, b, m, dopts)
    lst, lstats = sibeliaz_amd.JunctionStorage.load_device(graph, list(fasta), k, abundance=a, threads=2, stats=True, **jopts)
    got = _graph_of(lst)
    for key in got:
        assert got[key] == want[key], "%s: %s differs between lcb_graph_load_device and lcb_graph_load" % (what, key)
    lst.close()
    st, dev, stats = sibeliaz_amd.open_junctions(graph, list(fasta), k, sibeliaz_amd.Params.make(k, b=b, m=m), abundance=a, threads=2, stats=True, device_opts=dopts, **jopts)
    assert type(st) is sibeliaz_amd.JunctionStorage and type(dev) is sibeliaz_amd.Device
    got = _describe(st, dev)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], "%s: %s differs between lcb_open_junctions and the composed route" % (what, key)
    for s in (lstats, stats):
        assert s["kept_occurrences"] == yst.n_positions() and s["vertices"] == yst.GetVerticesNumber() and s["records"] == yst.GetChrNumber()
        assert s["raw_occurrences"] >= s["kept_occurrences"] and s["peak_device_bytes"] >= 12 * (os.path.getsize(graph) // 12) + 8 * s["raw_occurrences"]
        assert s["windows"] == s["table_slots"] == s["junction_kmers"] == s["partitions"] == 0 and s["insert_ms"] == s["emit_ms"] == s["mark_ms"] == 0
    assert stats["csr_ms"] == 0
    return st, dev, stats, yst


def _done(st, dev):
    dev.close()
    st.close()


# ---- the same graph and the same device

def test_file_opened_on_the_device_equals_the_loader_on_goldens(built, case):
    _done(*_check(case.graph, [case.fasta], case.k, case.a, case.name, b=case.b, m=case.m)[:2])        # (the committed file: the reference's ids)


@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_file_opened_on_the_device_equals_the_loader_on_edge_inputs(built, tmp_path, name):
    c = edge_inputs.build(name, str(tmp_path))
    st, dev, stats, _ = _check(c["graph"], c["fasta"], c["k"], c["a"], name, b=c["b"], m=c["m"])
    if name == "all_filtered":
        assert 0 < stats["kept_occurrences"] < stats["raw_occurrences"] // 2
    if name == "iupac_lowercase":
        assert stats["patched"] > 0
    _done(st, dev)


@pytest.mark.parametrize("params", seed_inputs.HEAVY)
def test_file_opened_on_the_device_equals_the_loader_on_heavy_inputs(built, tmp_path, params):
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    st, dev, stats, yst = _check(graph, [fasta], seed_inputs.K, seed_inputs.ABUNDANCE, "heavy%r" % (params,))
    seed_inputs.check_property(params, seed_inputs.ABUNDANCE, yst.seeds(2))
    if params[3]:
        assert stats["patched"] > 0
    _done(st, dev)


def test_file_opened_on_the_device_on_the_filtered_case_and_without_a_kept_position(built, tmp_path):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    st, dev, stats, yst = _check(graph, [fasta], seed_inputs.K, abundance, "heavy%r at abundance %d" % (params, abundance))
    seed_inputs.check_property(params, abundance, yst.seeds(2))
    assert 0 < stats["kept_occurrences"] < stats["raw_occurrences"]
    _done(st, dev)
    st, dev, stats, _ = _check(graph, [fasta], seed_inputs.K, 1, "abundance 1")               # K = 0
    assert stats["kept_occurrences"] == 0 < stats["raw_occurrences"] and stats["patched"] == 0 and len(dev.enumerate_seeds()) == 0
    _done(st, dev)


@pytest.mark.parametrize("name", file_inputs.LEGAL)
def test_file_opened_on_the_device_equals_the_loader_on_hand_packed_files(built, tmp_path, name):
    c = file_inputs.build(name, tmp_path)
    st, dev, stats, _ = _check(c["graph"], c["fasta"], c["k"], c["a"], name, tile_windows=file_inputs.TILE)
    assert stats["records"] == len(c["sizes"]) and stats["raw_occurrences"] == sum(c["sizes"])
    assert stats["tiles"] == (os.path.getsize(c["graph"]) // 12 + file_inputs.TILE - 1) // file_inputs.TILE
    if name in ("all_filtered", "separators_only", "empty"):
        assert stats["kept_occurrences"] == 0
    if name == "filtered_beyond_end":
        assert stats["kept_occurrences"] == stats["raw_occurrences"] - 4
    _done(st, dev)


# ---- tile sizes and layouts: the result never depends on them

LAYOUTS = [dict(seg_cap=64), dict(seg_cap=64, seg_gap=64), dict(seg_gap=1 << 20)]


def _ids(o):
    return "-".join("%s%d" % kv for kv in sorted(o.items())) or "default"


def _small(which, case_dir):
    """-> graph, fasta, k, a, b, m of a small input named `which`."""
    if which == "smallb":
        case = Case("smallb", case_dir)
        return case.graph, [case.fasta], case.k, case.a, case.b, case.m
    if which == "heavy_n":
        graph, f = seed_inputs.heavy(case_dir, *seed_inputs.HEAVY[6])
        return graph, [f], seed_inputs.K, seed_inputs.ABUNDANCE, 200, 50
    if which in file_inputs.LEGAL:
        c = file_inputs.build(which, case_dir)
    else:
        c = edge_inputs.build(which, case_dir)
    return c["graph"], c["fasta"], c["k"], c["a"], c["b"], c["m"]


@pytest.mark.parametrize("opts", [dict(tile_windows=64), dict(tile_windows=777), dict()], ids=_ids)
@pytest.mark.parametrize("which", ["smallb", "heavy_n", "long_chromosome"])
def test_the_result_does_not_depend_on_the_tile(built, case_dir, which, opts):
    graph, fasta, k, a, b, m = _small(which, case_dir)
    st, dev, stats, _ = _check(graph, fasta, k, a, "%s with %r" % (which, opts), b=b, m=m, **opts)
    n = os.path.getsize(graph) // 12
    if opts:
        assert stats["tiles"] == (n + opts["tile_windows"] - 1) // opts["tile_windows"] > 1
    else:
        assert stats["tiles"] == 1
    _done(st, dev)


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
@pytest.mark.parametrize("which", ["smallb", "iupac_lowercase", "filtered_beyond_end"])
def test_file_opened_on_the_device_under_segmented_layouts(built, case_dir, which, layout):
    graph, fasta, k, a, b, m = _small(which, case_dir)
    st, dev, stats, _ = _check(graph, fasta, k, a, "%s with %r" % (which, layout), b=b, m=m, dopts=layout)
    base = dev.read_table("seg_base")
    if "seg_cap" in layout:
        assert len(np.unique(base)) > 1, "one segment only"
    if layout.get("seg_gap"):          # placed by copies
        assert stats["place_ms"] > 0
    else:
        assert stats["place_ms"] == 0
    if which == "iupac_lowercase":
        assert stats["patched"] > 0 and stats["patch_ms"] > 0
    _done(st, dev)


def test_patches_reach_both_copies(built, tmp_path):
    c = edge_inputs.build("iupac_lowercase", str(tmp_path))
    yst = sibeliaz_amd.JunctionStorage(c["graph"], c["fasta"], c["k"], threads=2, abundance=c["a"])
    ydev = sibeliaz_amd.Device(yst, sibeliaz_amd.Params.make(c["k"]), 0, tables="host")
    want = ydev.read_table("pos_ch")
    ydev.close()
    st, dev, stats = sibeliaz_amd.open_junctions(c["graph"], c["fasta"], c["k"], sibeliaz_amd.Params.make(c["k"]), abundance=c["a"], threads=2, stats=True)
    got = dev.read_table("pos_ch")
    assert stats["patched"] > 0
    assert not (got == 0xFF).any(), "a sentinel byte is left in the device's posCh"
    assert got.tobytes() == want.tobytes()
    acgt = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    assert int((~np.isin(got, acgt)).sum()) == stats["patched"], "the letters outside ACGT are the patched ones"
    assert st.seeds(2).tobytes() == yst.seeds(2).tobytes()          # the host copy has them too: the host enumerator reads posCh of the storage
    _done(st, dev)
    yst.close()


# ---- through the engine and the CLI

def _blocks_text(blocks):
    return "".join("%d\t%d\t%d\t%d\n" % (int(b["id"]), int(b["chr"]), int(b["start"]), int(b["end"])) for b in blocks)


@pytest.mark.parametrize("seeds", ["host", "device"])
def test_find_blocks_on_the_pair_gives_the_committed_goldens(built, case, seeds):
    p = sibeliaz_amd.Params.make(case.k, b=case.b, m=case.m)
    st, dev = sibeliaz_amd.open_junctions(case.graph, [case.fasta], case.k, p, abundance=case.a, threads=2)
    finder = sibeliaz_amd.BlocksFinder(st, case.k)
    blocks = finder.FindBlocks(case.m, case.b, device=dev, threads=4, seeds=None if seeds == "host" else "device")
    summary = dict(ln.split("\t") for ln in case.golden("summary.txt").splitlines())
    assert _blocks_text(blocks) == case.golden("pretrim.tsv")
    assert finder.stats["blocks_found"] == int(summary["blocksFound"]) and finder.stats["failures"] == int(summary["failure"])
    _done(st, dev)


@pytest.mark.parametrize("seeds", ["host", "device"])
def test_cli_with_the_file_opened_on_the_device_writes_the_reference_gff(built, case, tmp_path, seeds):
    env = {k: v for k, v in os.environ.items() if k not in ("LCB_LOAD", "LCB_JUNCTIONS", "LCB_SEEDS", "LCB_TABLES", "LCB_GPUS", "LCB_VERBOSE", "LCB_HANDOVER")}

    def run(out, **extra):
        return subprocess.run([EXE, "--graph", case.graph, case.fasta, "-k", str(case.k), "-b", str(case.b), "-o", out, "-m", str(case.m), "-t", "4", "--abundance", str(case.a), "--noseq"],
                              capture_output=True, text=True, env=dict(env, **extra))
    want = run(str(tmp_path / "default"))
    got = run(str(tmp_path / "device"), LCB_LOAD="device", LCB_SEEDS=seeds, LCB_VERBOSE="1")
    assert want.returncode == 0 and got.returncode == 0, got.stderr
    assert got.stdout == want.stdout and "Blocks found:" in got.stdout          # the same banners
    assert "lcb: load=device chromosomes=" in got.stderr and "lcb: device tables=" not in got.stderr
    assert ("lcb: device seeds=" in got.stderr) == (seeds == "device")
    assert open(str(tmp_path / "device" / "blocks_coords.gff"), "rb").read() == case.golden("ref.gff", "rb")


# ---- errors and leftovers

def _free_bytes():
    """hipMemGetInfo's free bytes of device 0, asked of the HIP runtime the library itself is linked to."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipSetDevice(0) == 0 and hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_errors_have_the_loaders_text_and_leave_nothing_on_the_device(built, tmp_path):
    import ctypes as C
    lib = sibeliaz_amd.load_library()
    cases = [file_inputs.build(name, tmp_path) for name in sorted(file_inputs.ERRORS)]
    good = file_inputs.build("signed_ids", tmp_path)
    p = sibeliaz_amd.Params.make(file_inputs.K)

    def refused(c, **kw):
        with pytest.raises(sibeliaz_amd.LcbError) as want:
            sibeliaz_amd.JunctionStorage(c["graph"], c["fasta"], c["k"], threads=2, abundance=c["a"])
        assert str(want.value) == c["error"]
        with pytest.raises(sibeliaz_amd.LcbError) as got:
            sibeliaz_amd.JunctionStorage.load_device(c["graph"], c["fasta"], c["k"], abundance=c["a"], threads=2, **kw)
        assert str(got.value) == c["error"]
        with pytest.raises(sibeliaz_amd.LcbError) as got:
            sibeliaz_amd.open_junctions(c["graph"], c["fasta"], c["k"], p, abundance=c["a"], threads=2, **kw)
        assert str(got.value) == c["error"]
        arr = (C.c_char_p * 1)(os.fsencode(c["fasta"][0]))
        g, d = C.c_void_p(1), C.c_void_p(1)
        assert lib.lcb_open_junctions(os.fsencode(c["graph"]), arr, 1, c["k"], c["a"], 1, C.byref(p), 0, None, None, C.byref(g), C.byref(d), None) != 0
        assert g.value is None and d.value is None and lib.lcb_last_error().decode() == c["error"]

    # once untimed, so that whatever the runtime makes on first use exists; then the free bytes must come back
    _done(*sibeliaz_amd.open_junctions(good["graph"], good["fasta"], good["k"], p, abundance=good["a"], threads=2))
    refused(cases[0])
    before = _free_bytes()
    for c in cases:
        refused(c)
        refused(c, tile_windows=file_inputs.TILE)
    # a budget too small fails up front, naming the request, the budget and what is free
    with pytest.raises(sibeliaz_amd.LcbError) as e:
        sibeliaz_amd.open_junctions(good["graph"], good["fasta"], good["k"], p, abundance=good["a"], mem_budget=1 << 10)
    assert "lcb_open_junctions" in str(e.value) and " needs " in str(e.value) and "the budget is %d" % (1 << 10) in str(e.value) and "are free" in str(e.value)
    assert _free_bytes() == before, "device memory is left behind after refused calls"


def test_a_second_open_after_close_gives_the_same_bytes(built, tmp_path):
    c = file_inputs.build("long_chromosome", tmp_path)
    p = sibeliaz_amd.Params.make(c["k"])
    seen = []
    for _ in range(2):
        st, dev = sibeliaz_amd.open_junctions(c["graph"], c["fasta"], c["k"], p, abundance=c["a"], threads=2)
        seen.append(_describe(st, dev))
        dev.close()
        st.close()
    assert seen[0] == seen[1] and seen[0]["table pos_id"][1][0] > 0
