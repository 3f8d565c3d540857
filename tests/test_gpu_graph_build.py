"""GPU tests (-m gpu) of the graph build on the device (lcb_graph_build, JunctionStorage.build, LCB_JUNCTIONS=device; csrc/junctions.hip,
lcb_graph_kernels.h): the storage built from the FASTA files alone is the storage the two-step route gives - the CPU lcb-mkgraph writes a
junction file in the same test, lcb_graph_load reads it - on the goldens, the edge inputs and the heavy inputs; at the boundary of the
abundance filter; for every character case of posCh / posRevCh; across the blocks of the scan and the compaction; whatever the tile size,
the table capacity and the number of partitions; with the two-step route's error texts; through FindBlocks and the CLI. Exact comparisons only.

"The same graph": GetChrNumber and every chromosome's name and length, chr_start, pos_id, pos_pos, GetVerticesNumber, the host enumerator's
seeds, and all nine tables of a Device(..., tables="host") - which cover posCh, posRevCh and the host CSR."""
import os
import random
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from sibeliaz_amd import api
from tests import edge_inputs, seed_inputs
from tests.conftest import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sibeliaz_amd", "bin", "sibeliaz-lcb")
MKGRAPH = os.path.join(ROOT, "sibeliaz_amd", "bin", "lcb-mkgraph")
TABLE_NAMES = sorted(api.TABLES)
REC = np.dtype([("pos", "<u4"), ("id", "<i8")])


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mkgraph(fasta, k, out):
    """The yardstick's first step: the CPU tool."""
    if not os.path.exists(out):
        subprocess.check_call([MKGRAPH, "-k", str(k), "-o", out] + list(fasta), stderr=subprocess.DEVNULL)
    return out


def _raw(graph):
    """(records without the separators, the separators' indices) of a junction file."""
    r = np.fromfile(graph, dtype=REC)
    sep = (r["pos"] == 0xFFFFFFFF) | (r["id"] == np.iinfo(np.int64).max)
    return r[~sep], np.nonzero(sep)[0]


def _describe(st, k, b=200, m=50):
    """Everything "the same graph" compares, as a dict of bytes / values."""
    n = st.GetChrNumber()
    out = {"chromosomes": n, "names": [st.GetChrDescription(c) for c in range(n)], "lengths": [st.chr_len(c) for c in range(n)], "vertices": st.GetVerticesNumber(),
           "chr_start": st.chr_start().tobytes(), "pos_id": st.pos_id().tobytes(), "pos_pos": st.pos_pos().tobytes(), "seeds": st.seeds(2).tobytes()}
    dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(k, b=b, m=m), 0, tables="host")
    for name in TABLE_NAMES:
        t = dev.read_table(name)
        out["table " + name] = (str(t.dtype), t.shape, t.tobytes())
    dev.close()
    return out


_yard = {}


def _yardstick(graph, fasta, k, a):
    """The two-step route's storage and its description; computed once per input and left unchanged."""
    key = (graph, tuple(fasta), k, a)
    if key not in _yard:
        st = sibeliaz_amd.JunctionStorage(graph, list(fasta), k, threads=2, abundance=a)
        _yard[key] = (st, _describe(st, k))
    return _yard[key]


def _same_graph(built_st, want, k, what):
    got = _describe(built_st, k)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], "%s: %s differs between the device route and the two-step route" % (what, key)


def _check(graph, fasta, k, a, what, **opts):
    st, want = _yardstick(graph, fasta, k, a)
    built, stats = sibeliaz_amd.JunctionStorage.build(list(fasta), k, abundance=a, threads=2, stats=True, **opts)
    _same_graph(built, want, k, what)
    raw, _ = _raw(graph)
    assert stats["raw_occurrences"] == len(raw) == stats["occurrences"] == stats["junction_windows"]
    assert stats["kept_occurrences"] == st.n_positions() and stats["vertices"] == st.GetVerticesNumber() and stats["records"] == st.GetChrNumber()
    return built, stats, st


# ---- the same graph

def test_built_graph_equals_loaded_graph_on_goldens(built, case, tmp_path):
    graph = _mkgraph([case.fasta], case.k, str(tmp_path / "cpu.bin"))          # (the committed graph.bin has other ids)
    _check(graph, [case.fasta], case.k, case.a, case.name)


@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_built_graph_equals_loaded_graph_on_edge_inputs(built, tmp_path, name):
    c = edge_inputs.build(name, str(tmp_path))
    _, stats, st = _check(c["graph"], c["fasta"], c["k"], c["a"], name)
    if name == "all_filtered":
        assert 0 < stats["kept_occurrences"] < stats["raw_occurrences"] // 2
    if name == "iupac_lowercase":
        assert stats["patched"] > 0
    if name == "multi_file":
        assert len(c["fasta"]) > 1 and st.GetChrNumber() == 3


@pytest.mark.parametrize("params", seed_inputs.HEAVY)
def test_built_graph_equals_loaded_graph_on_heavy_inputs(built, tmp_path, params):
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    built_st, stats, st = _check(graph, [fasta], seed_inputs.K, seed_inputs.ABUNDANCE, "heavy%r" % (params,))
    seed_inputs.check_property(params, seed_inputs.ABUNDANCE, st.seeds(2))
    assert st.GetChrNumber() == params[1]
    if params[3]:
        assert stats["patched"] > 0 and (built_st.pos_id() < 0).any()


def test_built_graph_equals_loaded_graph_on_the_filtered_heavy_input(built, tmp_path):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    _, stats, st = _check(graph, [fasta], seed_inputs.K, abundance, "heavy%r at abundance %d" % (params, abundance))
    seed_inputs.check_property(params, abundance, st.seeds(2))
    assert 0 < stats["kept_occurrences"] < stats["raw_occurrences"]


# ---- the abundance boundary: abund[|id|] < abundance, counted over both strands and over the unfiltered input

def test_abundance_boundary(built, tmp_path):
    params = seed_inputs.HEAVY[1]
    n = params[0]                                                  # the junctions inside the repeat occur exactly n times
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    raw, _ = _raw(graph)
    ids = raw["id"].astype(np.int32).astype(np.int64)
    counts = np.bincount(np.abs(ids))
    exact = np.nonzero(counts == n)[0]
    assert len(exact) > 0, "no vertex occurs exactly %d times" % n
    both = [v for v in exact if (ids == v).any() and (ids == -v).any()]
    assert both, "no vertex whose %d occurrences are made of both strands" % n
    assert 0 < int((ids == both[0]).sum()) < n                     # neither strand reaches n alone
    kept = {}
    for a in (n, n + 1, 1):
        _, stats, _ = _check(graph, [fasta], seed_inputs.K, a, "abundance %d" % a)
        kept[a] = stats["kept_occurrences"]
        assert kept[a] == int((counts[np.abs(ids)] < a).sum())
    assert kept[1] == 0 < kept[n] < kept[n + 1] and kept[n + 1] - kept[n] == n * len(exact)


# ---- every character case of posCh / posRevCh in one FASTA

def test_character_cases(built, tmp_path):
    rng = random.Random(31)
    k = 15
    a, b, c, d = _rand(rng, 120), _rand(rng, 90), _rand(rng, 70), _rand(rng, 100)
    fasta = str(tmp_path / "chars.fa")
    with open(fasta, "w") as f:
        f.write(">one\n%sN%s\n%sr%s\n>two\n%s%s\n" % (a.lower(), b, c.lower(), d[:50], d, a[30:90]))
    graph = _mkgraph([fasta], k, str(tmp_path / "chars.bin"))
    built_st, stats, st = _check(graph, [fasta], k, 150, "character cases")
    seqs = ["".join(x.split("\n")[1:]).upper() for x in open(fasta).read().split(">")[1:]]
    cs, pos = st.chr_start().astype(np.int64), st.pos_pos().astype(np.int64)
    seen = set()
    to_patch = 0
    for ch in range(len(seqs)):
        s = seqs[ch]
        assert len(s) == st.chr_len(ch)
        for p in pos[cs[ch]:cs[ch + 1]]:
            if p == 0:
                seen.add("at position 0")
            if p + k == len(s):
                seen.add("window ends the record")
            elif s[p + k] == "N":
                seen.add("next base N")
            elif s[p + k] == "R":
                seen.add("next base R")
            if p + k < len(s) and s[p + k] not in "ACGT":
                to_patch += 1
            if p > 0 and s[p - 1] == "N":
                seen.add("previous base N")
    assert seen == {"at position 0", "window ends the record", "next base N", "next base R", "previous base N"}
    assert any(ch.islower() for ch in open(fasta).read().split("\n")[1])
    assert stats["patched"] == to_patch > 0
    # ... and the characters themselves, from the text (the tables of _check compared them with the two-step route's already)
    dev = sibeliaz_amd.Device(built_st, sibeliaz_amd.Params.make(k), 0, tables="host")
    got_ch, got_rev = dev.read_table("pos_ch"), dev.read_table("pos_rev_ch")
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for ch in range(len(seqs)):
        s = seqs[ch]
        for i in range(cs[ch], cs[ch + 1]):
            p = int(pos[i])
            assert got_ch[i] == (ord(s[p + k]) if p + k < len(s) else 0)
            assert got_rev[i] == ord(comp.get(s[p - 1], "N") if p > 0 else "N")


# ---- scan and compaction across their blocks

def _scan_text():
    """Random spacers of 6 bases between planted repeats of 16: 30 families of 300 copies and 100 families of 10 copies, dealt to six
    chromosomes of uneven sizes; a seventh, in the middle, is one frequent family in tandem and nothing else. The windows that lie in a
    repeat but for a base or two of a spacer are junctions too; at abundance 20 about half of all occurrences are filtered."""
    rng = random.Random(11)
    often, seldom = [_rand(rng, 16) for _ in range(30)], [_rand(rng, 16) for _ in range(100)]
    copies = [r for r in often for _ in range(300)] + [r for r in seldom for _ in range(10)]
    rng.shuffle(copies)
    cuts = [0, 1001, 3004, 4999, 6222, 8003, len(copies)]
    chrom = ["".join(_rand(rng, 6) + r for r in copies[cuts[i]:cuts[i + 1]]) + _rand(rng, 6) for i in range(6)]
    chrom.insert(3, often[0] * 130)
    return "".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(chrom))


def test_scan_and_compaction_across_blocks(built, tmp_path):
    k, a = 15, 20
    fasta = str(tmp_path / "scan.fa")
    with open(fasta, "w") as f:
        f.write(_scan_text())
    graph = _mkgraph([fasta], k, str(tmp_path / "scan.bin"))
    raw, sep = _raw(graph)
    assert len(raw) > 70000 > 256 * 256
    first = sep[:-1] - np.arange(len(sep) - 1)                     # raw index of the first record of chromosomes 1 ..
    assert len(sep) == 7 and (first % 256 != 0).all(), "a chromosome boundary falls on a block boundary"
    _, stats, st = _check(graph, [fasta], k, a, "scan input")
    assert 0.3 < stats["kept_occurrences"] / stats["raw_occurrences"] < 0.7
    sizes = np.diff(st.chr_start().astype(np.int64))
    assert sizes[3] == 0 and (np.delete(sizes, 3) > 256).all()
    assert first[3] - first[2] > 256, "the emptied chromosome spans no whole block of raw records"


# ---- sweeps: the graph never depends on the options

SWEEPS = [dict(tile_windows=64), dict(tile_windows=777), dict(tile_windows=1000), dict(tile_windows=4096), dict(table_log2=6), dict(partitions=1), dict(partitions=2),
          dict(partitions=3), dict(partitions=7), dict(partitions=3, tile_windows=777, table_log2=6), dict()]


@pytest.mark.parametrize("opts", SWEEPS, ids=lambda o: "-".join("%s%d" % kv for kv in sorted(o.items())) or "again")
@pytest.mark.parametrize("which", ["golden", "heavy"])
def test_graph_does_not_depend_on_the_options(built, case_dir, tmp_path_factory, which, opts):
    if which == "golden":
        case = Case("smallb", case_dir)
        fasta, k, a = case.fasta, case.k, case.a
        graph = _mkgraph([fasta], k, os.path.join(case_dir, "smallb_cpu.bin"))
    else:
        params, a = seed_inputs.FILTERED
        graph, fasta = seed_inputs.heavy(case_dir, *params)
        k = seed_inputs.K
    _, stats, _ = _check(graph, [fasta], k, a, "%s with %r" % (which, opts), **opts)
    if "table_log2" in opts:
        assert stats["table_rebuilds"] > 0
    if opts.get("tile_windows"):
        assert stats["tiles"] > 1
    assert stats["partitions"] == opts.get("partitions", 1)
    if opts.get("partitions", 1) > 1:
        assert stats["passes"] >= opts["partitions"] and stats["count_ms"] == 0


# ---- errors: the two-step route's texts

def _both_errors(tmp_path, name, text, k=15, extra=()):
    fasta = str(tmp_path / (name + ".fa"))
    with open(fasta, "w") as f:
        f.write(text)
    graph = _mkgraph([fasta], k, str(tmp_path / (name + ".bin")))
    files = [fasta] + list(extra)
    with pytest.raises(sibeliaz_amd.LcbError) as want:
        sibeliaz_amd.JunctionStorage(graph, files, k, threads=2, abundance=150)
    with pytest.raises(sibeliaz_amd.LcbError) as got:
        sibeliaz_amd.JunctionStorage.build(files, k, abundance=150, threads=2)
    assert str(got.value) == str(want.value)
    return str(got.value)


def test_errors_have_the_two_step_routes_text(built, tmp_path):
    rng = random.Random(8)
    s, t = _rand(rng, 300), _rand(rng, 200)
    assert "chromosome without junctions" in _both_errors(tmp_path, "short_first", ">a\n%s\n>short\nACGTACG\n>b\n%s\n" % (s, t))
    assert "more records" in _both_errors(tmp_path, "short_last", ">a\n%s\n>b\n%s\n>short\nACGTACG\n" % (s, t))
    assert "invalid character '#'" in _both_errors(tmp_path, "hash", ">a\n%s\n>b\n%s#%s\n" % (s, t[:100], t[100:]))
    missing = str(tmp_path / "missing.fa")
    assert _both_errors(tmp_path, "one_good", ">a\n%s\n" % s, extra=[missing]) == "Can't open file " + missing
    # ... and a failed build leaves nothing on the device: the next one runs
    st = sibeliaz_amd.JunctionStorage.build([str(tmp_path / "one_good.fa")], 15)
    assert st.GetChrNumber() == 1 and st.n_positions() >= 2


# ---- end to end

def _blocks_text(blocks):
    return "".join("%d\t%d\t%d\t%d\n" % (int(b["id"]), int(b["chr"]), int(b["start"]), int(b["end"])) for b in blocks)


def test_find_blocks_on_the_built_storage(built, case_dir):
    case = Case("smallb", case_dir)
    graph = _mkgraph([case.fasta], case.k, os.path.join(case_dir, "smallb_cpu.bin"))
    file_st = sibeliaz_amd.JunctionStorage(graph, [case.fasta], case.k, threads=2, abundance=case.a)
    built_st = sibeliaz_amd.JunctionStorage.build([case.fasta], case.k, abundance=case.a, threads=2)
    want = sibeliaz_amd.BlocksFinder(file_st, case.k).FindBlocks(case.m, case.b, threads=2)
    got = sibeliaz_amd.BlocksFinder(built_st, case.k).FindBlocks(case.m, case.b, threads=2)
    assert len(want) > 0 and _blocks_text(got) == _blocks_text(want)


@pytest.mark.parametrize("routes", [{}, {"LCB_SEEDS": "device", "LCB_TABLES": "device"}], ids=["alone", "with_device_seeds_and_tables"])
def test_cli_with_device_junctions_writes_the_file_routes_output(built, case_dir, tmp_path, routes):
    case = Case("smallb", case_dir)
    graph = _mkgraph([case.fasta], case.k, os.path.join(case_dir, "smallb_cpu.bin"))
    env = {k: v for k, v in os.environ.items() if k not in ("LCB_JUNCTIONS", "LCB_SEEDS", "LCB_TABLES", "LCB_GPUS", "LCB_VERBOSE")}

    def run(graph_arg, out, **extra):
        return subprocess.run([EXE, "--graph", graph_arg, case.fasta, "-k", str(case.k), "-b", str(case.b), "-o", out, "-m", str(case.m), "-t", "4", "--abundance", str(case.a), "--chunks", "3"],
                              capture_output=True, text=True, env=dict(env, **extra))
    want = run(graph, str(tmp_path / "file"))
    missing = str(tmp_path / "no_such_graph.bin")
    got = run(missing, str(tmp_path / "device"), LCB_JUNCTIONS="device", LCB_VERBOSE="1", **routes)
    assert want.returncode == 0 and got.returncode == 0, got.stderr
    assert got.stdout == want.stdout and "Blocks found:" in got.stdout
    assert "lcb: graph=device records=" in got.stderr and not os.path.exists(missing)
    def tree(top):          # every file under top (the block sequences too: they come from the graph's strings) -> its bytes
        return {os.path.relpath(os.path.join(d, fn), top): open(os.path.join(d, fn), "rb").read() for d, _, files in os.walk(top) for fn in files}
    files, dev_files = tree(str(tmp_path / "file")), tree(str(tmp_path / "device"))
    assert "blocks_coords.gff" in files and len(files) > 1 and sorted(files) == sorted(dev_files)
    for fn in files:
        assert dev_files[fn] == files[fn], fn


# ---- stats

def test_stats_account_for_the_download_and_the_device_memory(built, tmp_path):
    params, abundance = seed_inputs.FILTERED
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    built_st, stats = sibeliaz_amd.JunctionStorage.build([fasta], seed_inputs.K, abundance=abundance, stats=True)
    kept, raw, n_chr = stats["kept_occurrences"], stats["raw_occurrences"], built_st.GetChrNumber()
    assert kept == built_st.n_positions() > 0
    assert stats["download_bytes"] == 10 * kept + 16 * n_chr + 16
    seq_bytes = sum(built_st.chr_len(c) for c in range(n_chr)) + n_chr + 1
    # what is live at the compaction
    formula = seq_bytes + 64 + 8 * raw + 4 * (stats["vertices"] + 1) + 10 * kept + 8 * (2 * (n_chr + 1) + (n_chr + 1) + ((raw + 255) // 256 + 1) + 2)
    assert stats["peak_device_bytes"] >= formula
    # the budget is compared before anything is allocated, and the message names both numbers
    with pytest.raises(sibeliaz_amd.LcbError) as e:
        sibeliaz_amd.JunctionStorage.build([fasta], seed_inputs.K, abundance=abundance, mem_budget=1 << 16)
    assert "lcb_graph_build" in str(e.value) and str(1 << 16) in str(e.value)
