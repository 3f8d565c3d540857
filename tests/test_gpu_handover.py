"""GPU tests (-m gpu) of the hand-over route (lcb_open_fasta, sibeliaz_amd.open_fasta, LCB_HANDOVER=device; csrc/junctions.hip, device.hip,
tables.hip, lcb_handover_kernels.h): one call from the FASTA files gives the storage of the two-step route - the CPU lcb-mkgraph writes a
junction file in the same test, JunctionStorage reads it - and a device whose nine tables are those of Device(yardstick, params,
tables="host") with the same device options; under segmented layouts with and without a gap; whatever the junction options; with the
patched letters in both copies; without the bytes that no longer cross the bus; through FindBlocks and the CLI; with the two-step
route's error texts and nothing left behind. Exact comparisons only."""
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests import edge_inputs, seed_inputs
from tests.conftest import Case
from tests.test_handover_emu import emptied_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sibeliaz_amd", "bin", "sibeliaz-lcb")
MKGRAPH = os.path.join(ROOT, "sibeliaz_amd", "bin", "lcb-mkgraph")
TABLE_NAMES = sorted(api.TABLES)


def _mkgraph(fasta, k, out):
    """The yardstick's first step: the CPU tool."""
    if not os.path.exists(out):
        subprocess.check_call([MKGRAPH, "-k", str(k), "-o", out] + list(fasta), stderr=subprocess.DEVNULL)
    return out


def _describe(st, dev):
    """Everything "the same graph and the same device" compares, as a dict of bytes / values."""
    n = st.GetChrNumber()
    out = {"chromosomes": n, "names": [st.GetChrDescription(c) for c in range(n)], "lengths": [st.chr_len(c) for c in range(n)], "vertices": st.GetVerticesNumber(),
           "chr_start": st.chr_start().tobytes(), "pos_id": st.pos_id().tobytes(), "pos_pos": st.pos_pos().tobytes(), "seeds": st.seeds(2).tobytes()}
    for name in TABLE_NAMES:
        t = dev.read_table(name)
        out["table " + name] = (str(t.dtype), t.shape, t.tobytes())
    return out


_yard = {}


def _yardstick(graph, fasta, k, a, b, m, dopts):
    """The two-step route's storage, the description of it and of a host-route device with the same options; computed once per input
    and layout and left unchanged."""
    key = (graph, tuple(fasta), k, a, b, m, tuple(sorted(dopts.items())))
    if key not in _yard:
        skey = (graph, tuple(fasta), k, a)
        if skey not in _yard:
            _yard[skey] = sibeliaz_amd.JunctionStorage(graph, list(fasta), k, threads=2, abundance=a)
        st = _yard[skey]
        dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(k, b=b, m=m), 0, tables="host", **dopts)
        _yard[key] = (st, _describe(st, dev))
        dev.close()
    return _yard[key]


def _check(graph, fasta, k, a, what, b=200, m=50, dopts=None, **jopts):
    """open_fasta against the yardstick -> (storage, device, stats, the yardstick's storage); the caller closes device, then storage."""
    dopts = dopts or {}
    yst, want = _yardstick(graph, fasta, k, a, b, m, dopts)
    st, dev, stats = sibeliaz_amd.open_fasta(list(fasta), k, sibeliaz_amd.Params.make(k, b=b, m=m), abundance=a, threads=2, stats=True, device_opts=dopts, **jopts)
    assert type(st) is sibeliaz_amd.JunctionStorage and type(dev) is sibeliaz_amd.Device
    got = _describe(st, dev)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], "%s: %s differs between the hand-over route and the two-step route" % (what, key)
    assert dev.enumerate_seeds().tobytes() == yst.seeds(2).tobytes(), "%s: the device's seeds differ from the host enumerator's" % what
    kept, vertices, q = stats["kept_occurrences"], stats["vertices"], 8 if (dopts.get("seg_cap") or len(np.unique(dev.read_table("seg_base"))) > 1) else 4
    assert kept == yst.n_positions() and vertices == yst.GetVerticesNumber() and stats["records"] == yst.GetChrNumber()
    assert stats["csr_ms"] == 0
    assert stats["csr_download_bytes"] == (q + 4) * kept + q * (vertices + 1)
    assert stats["download_bytes"] == 10 * kept + 16 * yst.GetChrNumber() + 16
    assert stats["peak_device_bytes"] >= stats["device_bytes"] + 14 * kept
    return st, dev, stats, yst


def _done(st, dev):
    dev.close()
    st.close()


# ---- the same graph and the same device

def test_open_fasta_equals_the_two_steps_on_goldens(built, case, case_dir):
    graph = _mkgraph([case.fasta], case.k, os.path.join(case_dir, case.name + "_cpu.bin"))          # (the committed graph.bin has other ids)
    _done(*_check(graph, [case.fasta], case.k, case.a, case.name, b=case.b, m=case.m)[:2])


@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_open_fasta_equals_the_two_steps_on_edge_inputs(built, tmp_path, name):
    c = edge_inputs.build(name, str(tmp_path))
    st, dev, stats, _ = _check(c["graph"], c["fasta"], c["k"], c["a"], name, b=c["b"], m=c["m"])
    if name == "all_filtered":
        assert 0 < stats["kept_occurrences"] < stats["raw_occurrences"] // 2
    if name == "iupac_lowercase":
        assert stats["patched"] > 0
    _done(st, dev)


def test_open_fasta_with_an_emptied_chromosome(built, tmp_path):
    graph, fasta = seed_inputs.write_input(tmp_path, "emptied", emptied_text())
    st, dev, stats, _ = _check(graph, [fasta], seed_inputs.K, 20, "emptied chromosome")
    sizes = np.diff(st.chr_start().astype(np.int64))
    assert sizes[1] == 0 and sizes[0] > 0 and sizes[2] > 0
    _done(st, dev)


@pytest.mark.parametrize("params", seed_inputs.HEAVY)
def test_open_fasta_equals_the_two_steps_on_heavy_inputs(built, tmp_path, params):
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    st, dev, stats, yst = _check(graph, [fasta], seed_inputs.K, seed_inputs.ABUNDANCE, "heavy%r" % (params,))
    seed_inputs.check_property(params, seed_inputs.ABUNDANCE, yst.seeds(2))
    # what did not cross the bus: the table step uploads the segment plan and the patch list, not 10 bytes per occurrence
    # (it uploads 28 bytes per chromosome, 264 of segment bases and sums, 9 per patch: below 10 per occurrence from 30 occurrences per chromosome on)
    wide_margin = stats["kept_occurrences"] > 30 * st.GetChrNumber() + 30 + stats["patched"]
    assert wide_margin or params[1] >= 300
    if wide_margin:
        assert stats["upload_bytes"] < 10 * stats["kept_occurrences"]
    if params[3]:
        assert stats["patched"] > 0
    _done(st, dev)


def test_open_fasta_on_the_filtered_case_and_without_a_kept_position(built, tmp_path):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    st, dev, stats, yst = _check(graph, [fasta], seed_inputs.K, abundance, "heavy%r at abundance %d" % (params, abundance))
    seed_inputs.check_property(params, abundance, yst.seeds(2))
    assert 0 < stats["kept_occurrences"] < stats["raw_occurrences"]
    _done(st, dev)
    st, dev, stats, _ = _check(graph, [fasta], seed_inputs.K, 1, "abundance 1")               # K = 0
    assert stats["kept_occurrences"] == 0 < stats["raw_occurrences"] and stats["patched"] == 0 and len(dev.enumerate_seeds()) == 0
    _done(st, dev)


# ---- layouts and option sweeps: the result never depends on them

LAYOUTS = [dict(seg_cap=64), dict(seg_cap=64, seg_gap=64), dict(seg_gap=1 << 20)]
SWEEPS = [dict(tile_windows=64), dict(tile_windows=777), dict(table_log2=6), dict(partitions=1), dict(partitions=2), dict(partitions=3), dict(partitions=3, tile_windows=777, table_log2=6)]


def _ids(o):
    return "-".join("%s%d" % kv for kv in sorted(o.items()))


@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
@pytest.mark.parametrize("which", ["smallb", "iupac_lowercase", "multi_file", "heavy_n", "emptied"])
def test_open_fasta_under_segmented_layouts(built, case_dir, tmp_path_factory, which, layout):
    """seg_cap=64: several segments (a chromosome of more than 64 positions is a segment of its own), the 64-bit payloads; with a gap
    the arrays are placed segment by segment, device to device, and a patch lands at a shifted index."""
    b, m = 200, 50
    if which == "smallb":
        case = Case("smallb", case_dir)
        fasta, k, a, b, m = [case.fasta], case.k, case.a, case.b, case.m
        graph = _mkgraph(fasta, k, os.path.join(case_dir, "smallb_cpu.bin"))
    elif which == "heavy_n":
        graph, f = seed_inputs.heavy(case_dir, *seed_inputs.HEAVY[6])
        fasta, k, a = [f], seed_inputs.K, seed_inputs.ABUNDANCE
    elif which == "emptied":
        graph, f = seed_inputs.write_input(case_dir, "emptied", emptied_text())
        fasta, k, a = [f], seed_inputs.K, 20
    else:
        c = edge_inputs.build(which, case_dir)
        graph, fasta, k, a, b, m = c["graph"], c["fasta"], c["k"], c["a"], c["b"], c["m"]
    st, dev, stats, _ = _check(graph, fasta, k, a, "%s with %r" % (which, layout), b=b, m=m, dopts=layout)
    base = dev.read_table("seg_base")
    if "seg_cap" in layout:
        assert len(np.unique(base)) > 1, "one segment only"
    if layout.get("seg_gap"):          # placed by copies; a second segment begins a gap further on
        assert stats["place_ms"] > 0
        if len(np.unique(base)) > 1:
            assert int(base.max()) >= layout["seg_gap"] + 64
    else:
        assert stats["place_ms"] == 0
    if which in ("iupac_lowercase", "heavy_n"):
        assert stats["patched"] > 0 and stats["patch_ms"] > 0
    _done(st, dev)


@pytest.mark.parametrize("opts", SWEEPS, ids=_ids)
@pytest.mark.parametrize("which", ["golden", "heavy"])
def test_open_fasta_does_not_depend_on_the_junction_options(built, case_dir, which, opts):
    if which == "golden":
        case = Case("smallb", case_dir)
        fasta, k, a, b, m = case.fasta, case.k, case.a, case.b, case.m
        graph = _mkgraph([fasta], k, os.path.join(case_dir, "smallb_cpu.bin"))
    else:
        (params, a), b, m = seed_inputs.FILTERED, 200, 50
        graph, fasta = seed_inputs.heavy(case_dir, *params)
        k = seed_inputs.K
    st, dev, stats, _ = _check(graph, [fasta], k, a, "%s with %r" % (which, opts), b=b, m=m, **opts)
    if "table_log2" in opts:
        assert stats["table_rebuilds"] > 0
    if opts.get("tile_windows"):
        assert stats["tiles"] > 1
    assert stats["partitions"] == opts.get("partitions", 1)
    _done(st, dev)


# ---- patches reach both copies

@pytest.mark.parametrize("which", ["iupac_lowercase", "heavy_n"])
def test_patches_reach_both_copies(built, tmp_path, which):
    if which == "heavy_n":
        graph, f = seed_inputs.heavy(tmp_path, *seed_inputs.HEAVY[6])
        fasta, k, a = [f], seed_inputs.K, seed_inputs.ABUNDANCE
    else:
        c = edge_inputs.build(which, str(tmp_path))
        graph, fasta, k, a = c["graph"], c["fasta"], c["k"], c["a"]
    yst = sibeliaz_amd.JunctionStorage(graph, list(fasta), k, threads=2, abundance=a)
    ydev = sibeliaz_amd.Device(yst, sibeliaz_amd.Params.make(k), 0, tables="host")
    want = ydev.read_table("pos_ch")
    ydev.close()
    st, dev, stats = sibeliaz_amd.open_fasta(list(fasta), k, sibeliaz_amd.Params.make(k), abundance=a, threads=2, stats=True)
    got = dev.read_table("pos_ch")
    assert stats["patched"] > 0
    assert not (got == 0xFF).any(), "a sentinel byte is left in the device's posCh"
    assert got.tobytes() == want.tobytes()
    acgt = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    assert int((~np.isin(got, acgt)).sum()) == stats["patched"], "the letters outside ACGT are the patched ones"
    # the host copy has them too: the host enumerator reads posCh of the storage
    assert st.seeds(2).tobytes() == yst.seeds(2).tobytes()
    _done(st, dev)
    yst.close()


# ---- through the engine and the CLI

def _blocks_text(blocks):
    return "".join("%d\t%d\t%d\t%d\n" % (int(b["id"]), int(b["chr"]), int(b["start"]), int(b["end"])) for b in blocks)


@pytest.mark.parametrize("seeds", ["host", "device"])
def test_find_blocks_on_the_pair_gives_the_committed_goldens(built, case, seeds):
    p = sibeliaz_amd.Params.make(case.k, b=case.b, m=case.m)
    st, dev = sibeliaz_amd.open_fasta([case.fasta], case.k, p, abundance=case.a, threads=2)
    finder = sibeliaz_amd.BlocksFinder(st, case.k)
    blocks = finder.FindBlocks(case.m, case.b, device=dev, threads=4, seeds=None if seeds == "host" else "device")
    summary = dict(ln.split("\t") for ln in case.golden("summary.txt").splitlines())
    print("blocks %d golden lines %d blocks_found %d / %s failures %d / %s" % (len(blocks), len(case.golden("pretrim.tsv").splitlines()), finder.stats["blocks_found"], summary["blocksFound"],
                                                                          finder.stats["failures"], summary["failure"]))
    assert _blocks_text(blocks) == case.golden("pretrim.tsv")
    assert finder.stats["blocks_found"] == int(summary["blocksFound"]) and finder.stats["failures"] == int(summary["failure"])
    _done(st, dev)


@pytest.mark.parametrize("seeds", ["host", "device"])
def test_cli_with_the_handover_writes_the_reference_gff(built, case, tmp_path, seeds):
    env = {k: v for k, v in os.environ.items() if k not in ("LCB_JUNCTIONS", "LCB_SEEDS", "LCB_TABLES", "LCB_GPUS", "LCB_VERBOSE", "LCB_HANDOVER")}

    def run(graph_arg, out, **extra):
        return subprocess.run([EXE, "--graph", graph_arg, case.fasta, "-k", str(case.k), "-b", str(case.b), "-o", out, "-m", str(case.m), "-t", "4", "--abundance", str(case.a), "--noseq"],
                              capture_output=True, text=True, env=dict(env, **extra))
    want = run(case.graph, str(tmp_path / "default"))
    got = run("unused", str(tmp_path / "handover"), LCB_JUNCTIONS="device", LCB_HANDOVER="device", LCB_SEEDS=seeds, LCB_VERBOSE="1")
    assert want.returncode == 0 and got.returncode == 0, got.stderr
    assert got.stdout == want.stdout and "Blocks found:" in got.stdout          # the same banners
    assert "lcb: handover=device records=" in got.stderr and "lcb: graph=device" not in got.stderr and not os.path.exists("unused")
    assert ("lcb: device seeds=" in got.stderr) == (seeds == "device")
    assert open(str(tmp_path / "handover" / "blocks_coords.gff"), "rb").read() == case.golden("ref.gff", "rb")


# ---- errors and leftovers

def test_errors_have_the_two_step_routes_text_and_leave_no_device(built, tmp_path):
    lib = sibeliaz_amd.load_library()
    fasta = str(tmp_path / "hash.fa")
    s = "ACGTTGCAAGCTTAGCCGATAGCTAGGATCCGATTACGATCGGCTAAGCTTCGATCGATTAGC" * 4
    with open(fasta, "w") as f:
        f.write(">a\n%s\n>b\n%s#%s\n" % (s, s[:100], s[100:]))
    graph = _mkgraph([fasta], 15, str(tmp_path / "hash.bin"))
    with pytest.raises(sibeliaz_amd.LcbError) as want:
        sibeliaz_amd.JunctionStorage(graph, [fasta], 15, threads=2, abundance=150)
    with pytest.raises(sibeliaz_amd.LcbError) as got:
        sibeliaz_amd.open_fasta([fasta], 15, sibeliaz_amd.Params.make(15), threads=2)
    assert str(got.value) == str(want.value) and "invalid character '#'" in str(got.value)
    import ctypes as C
    arr = (C.c_char_p * 1)(os.fsencode(fasta))
    g, d = C.c_void_p(1), C.c_void_p(1)
    p = sibeliaz_amd.Params.make(15)
    assert lib.lcb_open_fasta(arr, 1, 15, 150, 1, C.byref(p), 0, None, None, C.byref(g), C.byref(d), None) != 0 and g.value is None and d.value is None
    # a budget too small for the junction part fails up front, with both numbers
    graph, good = seed_inputs.heavy(tmp_path, *seed_inputs.HEAVY[3])
    with pytest.raises(sibeliaz_amd.LcbError) as e:
        sibeliaz_amd.open_fasta([good], seed_inputs.K, sibeliaz_amd.Params.make(seed_inputs.K), abundance=seed_inputs.ABUNDANCE, mem_budget=1 << 16)
    assert "lcb_open_fasta" in str(e.value) and str(1 << 16) in str(e.value) and "needs" in str(e.value)


def test_a_second_open_after_close_gives_the_same_bytes(built, tmp_path):
    graph, fasta = seed_inputs.heavy(tmp_path, *seed_inputs.HEAVY[6])
    p = sibeliaz_amd.Params.make(seed_inputs.K)
    seen = []
    for _ in range(2):
        st, dev = sibeliaz_amd.open_fasta([fasta], seed_inputs.K, p, abundance=seed_inputs.ABUNDANCE, threads=2)
        seen.append(_describe(st, dev))
        dev.close()
        st.close()
    assert seen[0] == seen[1] and seen[0]["table pos_id"][1][0] > 0
