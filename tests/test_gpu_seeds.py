"""GPU tests (-m gpu) of the seed enumeration and ordering on the device (csrc/seeds.hip, lcb_seed_kernels.h): lcb_device_enumerate_seeds
gives the host enumerator's array - and through it the sha256 of the REAL reference's sorted bundle_ - on the goldens, on segmented
device tables, on the edge inputs, and on synthetic inputs whose occurrence lists span several 64-occurrence chunks;
lcb_device_sort_seeds orders generated keys as Bundle::operator< does; and the device is left as it was. Exact comparisons only."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from tests import edge_inputs, seed_inputs
from tests.test_gpu_parity import _setup
from tests.test_gpu_segments import _seg_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024          # S_TILE of lcb_seed_kernels.h
FIELDS = ("vid", "ch", "count", "rank", "resolve_pos", "resolve_chr")


def _same(got, want, what):
    assert got.dtype == sibeliaz_amd.SEED_DTYPE and len(got) == len(want), "%s: %d seeds, the host has %d" % (what, len(got), len(want))
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, "%s: field %s differs first at seed %d: device %r, host %r" % (what, f, bad[0], got[bad[0]], want[bad[0]])


def _text(seeds):
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\n" % (int(s["vid"]), int(s["ch"]), int(s["count"]), int(s["rank"]), int(s["resolve_pos"]), int(s["resolve_chr"])) for s in seeds)


def test_device_seeds_match_golden_and_host(built, case):
    st, p, dev = _setup(case)
    got, stats = dev.enumerate_seeds(stats=True)
    assert hashlib.sha256(_text(got).encode()).hexdigest() == case.meta["sha256"]["bundles.tsv"]     # the REAL reference's sorted bundle_
    want = st.seeds(4)
    _same(got, want, case.name)
    _same(dev.enumerate_seeds(), want, case.name + ", second call")
    assert stats["seeds"] == len(want) and stats["vertices"] == st.GetVerticesNumber() and stats["max_count"] == int(want["count"].max())
    assert stats["sort_passes"] + stats["sort_passes_skipped"] == 19 and stats["sort_passes_skipped"] >= 3      # the high bytes of count
    assert stats["device_bytes"] >= 48 * len(want)


@pytest.mark.parametrize("flavour", ["many", "gap"])
def test_device_seeds_on_segmented_tables(built, case, flavour):
    st, p, dev = _seg_setup(case, flavour)
    _same(dev.enumerate_seeds(), st.seeds(4), "%s, segments (%s)" % (case.name, flavour))


def test_device_seeds_with_flat_indices_beyond_32_bits(built, case_dir):
    from tests.conftest import Case
    case = Case("twogenomes", case_dir)
    st, p, dev = _seg_setup(case, "wide")
    _same(dev.enumerate_seeds(), st.seeds(4), "twogenomes, segments (wide)")


@pytest.mark.parametrize("name", edge_inputs.NAMES)
def test_device_seeds_on_edge_inputs(built, tmp_path, name):
    c = edge_inputs.build(name, str(tmp_path))
    st = sibeliaz_amd.JunctionStorage(c["graph"], c["fasta"], c["k"], threads=2, abundance=c["a"])
    dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(c["k"], b=c["b"], m=c["m"]), 0)
    got = dev.enumerate_seeds()
    _same(got, st.seeds(2), name)
    if name == "all_filtered":
        assert len(got) == 0
    # (single_strain is not seedless: one 15-mer of its 6000 random bases repeats, and the host enumerator finds the seed
    # (-2, 'T', count 2) too. The input without any seed is the next test's.)


def test_device_seeds_of_an_input_without_seeds(built, tmp_path):
    graph, fasta = seed_inputs.no_seed(tmp_path)
    st = sibeliaz_amd.JunctionStorage(graph, [fasta], seed_inputs.K, threads=1, abundance=seed_inputs.ABUNDANCE)
    assert len(st.seeds(1)) == 0
    dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(seed_inputs.K, b=200, m=50), 0)
    got, stats = dev.enumerate_seeds(stats=True)
    assert got.dtype == sibeliaz_amd.SEED_DTYPE and len(got) == 0
    assert stats["seeds"] == 0 and stats["max_count"] == 0 and stats["sort_passes"] == 0


@pytest.mark.parametrize("params,abundance", [(p, seed_inputs.ABUNDANCE) for p in seed_inputs.HEAVY] + [seed_inputs.FILTERED],
                         ids=lambda v: "heavy_%d_%d_%d_%d" % v if isinstance(v, tuple) else "a%d" % v)
def test_device_seeds_on_long_lists(built, tmp_path, params, abundance):
    graph, fasta = seed_inputs.heavy(tmp_path, *params)
    st = sibeliaz_amd.JunctionStorage(graph, [fasta], seed_inputs.K, threads=2, abundance=abundance)
    want = st.seeds(2)
    seed_inputs.check_property(params, abundance, want)
    dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(seed_inputs.K, b=200, m=50), 0)
    got, stats = dev.enumerate_seeds(stats=True)
    _same(got, want, "heavy%r at abundance %d" % (params, abundance))
    assert stats["max_count"] == int(want["count"].max())


# ---- lcb_device_sort_seeds ------------------------------------------------------------------------------------------------------------
def _keys(n, pattern):
    rng = np.random.default_rng(12345 + n)
    s = np.zeros(n, dtype=sibeliaz_amd.SEED_DTYPE)
    s["vid"] = np.arange(n)                       # a key that ties shows an unstable pass
    s["ch"] = -3                                  # (not a byte's worth: vid and ch travel untouched)
    s["count"], s["rank"], s["resolve_pos"], s["resolve_chr"] = 7, 1000, 100, 5
    u64 = lambda: rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if pattern == "random":
        s["count"], s["rank"], s["resolve_pos"], s["resolve_chr"] = u64() >> np.uint64(32), u64(), u64() >> np.uint64(32), u64() >> np.uint64(40)
    elif pattern == "count_top":
        s["count"] = (u64() & np.uint64(255)) << np.uint64(24)
    elif pattern == "chr_only":
        s["resolve_chr"] = u64() >> np.uint64(40)
    elif pattern == "rank_low":
        s["rank"] = np.uint64(0x1234567800) | (u64() & np.uint64(255))
    elif pattern == "rank_wrap":
        s["rank"] = np.uint64(1 << 63) + rng.integers(-1000, 1001, n).astype(np.int64).view(np.uint64)
    elif pattern == "count_equal":
        s["count"], s["rank"], s["resolve_pos"] = 42, u64(), u64() >> np.uint64(32)
    return s


def _host_order(s):
    # Bundle::operator<: count descending, then rank, resolve_pos, resolve_chr ascending; stable
    return s[np.lexsort((s["resolve_chr"], s["resolve_pos"], s["rank"], np.uint64(0xFFFFFFFF) - s["count"]))]


@pytest.fixture(scope="module")
def sort_device(built, tmp_path_factory):
    graph, fasta = seed_inputs.no_seed(tmp_path_factory.mktemp("sort"))
    st = sibeliaz_amd.JunctionStorage(graph, [fasta], seed_inputs.K, threads=1, abundance=seed_inputs.ABUNDANCE)
    return sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(seed_inputs.K, b=200, m=50), 0)


@pytest.mark.parametrize("pattern", ["random", "count_top", "chr_only", "rank_low", "rank_wrap", "count_equal"])
def test_device_sort_orders_generated_keys(sort_device, pattern):
    for n in (0, 1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 17):
        s = _keys(n, pattern)
        before = s.copy()
        got = sort_device.sort_seeds(s)
        assert s.tobytes() == before.tobytes(), "sort_seeds changed its argument"
        assert got.tobytes() == _host_order(s).tobytes(), "%s, n = %d" % (pattern, n)


def test_device_sort_restores_a_shuffled_seed_list_and_checks_ranges(built, case_dir):
    from tests.conftest import Case
    case = Case("smallb", case_dir)
    st, p, dev = _setup(case)
    want = st.seeds(4)
    shuffled = want[np.random.default_rng(3).permutation(len(want))]
    assert shuffled.tobytes() != want.tobytes()
    assert dev.sort_seeds(shuffled).tobytes() == want.tobytes()
    for field, value in (("resolve_chr", 1 << 24), ("resolve_pos", 1 << 32), ("count", 1 << 32)):
        bad = want[:5].copy()
        bad[field][3] = value
        with pytest.raises(sibeliaz_amd.LcbError, match="seed 3"):
            dev.sort_seeds(bad)


# ---- the device is left as it was -----------------------------------------------------------------------------------------------------
def test_enumeration_leaves_the_device_as_it_was(built, case_dir, tmp_path):
    from tests.conftest import Case
    case = Case("smallb", case_dir)
    st, p, dev = _setup(case)
    seeds = st.seeds(4)[:256]
    dev.mark_used([[10, 200]])
    off, inst, score, _ = dev.process_seeds(seeds)
    _same(dev.enumerate_seeds()[:256], seeds, "smallb with marked positions")
    off2, inst2, score2, _ = dev.process_seeds(seeds)
    assert off.tobytes() == off2.tobytes() and inst.tobytes() == inst2.tobytes() and score.tobytes() == score2.tobytes()
    dev.reset_used()
    finder = sibeliaz_amd.BlocksFinder(st, case.k)
    blocks = finder.FindBlocks(case.m, case.b, device=dev, seeds="device")
    text = "".join("%d\t%d\t%d\t%d\n" % (int(b["id"]), int(b["chr"]), int(b["start"]), int(b["end"])) for b in blocks)
    assert hashlib.sha256(text.encode()).hexdigest() == hashlib.sha256(case.golden("pretrim.tsv").encode()).hexdigest()


def test_cli_with_device_seeds_writes_the_reference_file(built, case_dir, tmp_path):
    from tests.conftest import Case
    case = Case("smallb", case_dir)
    out = str(tmp_path / "cli")
    r = subprocess.run([os.path.join(ROOT, "sibeliaz_amd", "bin", "sibeliaz-lcb"), "--graph", case.graph, case.fasta, "-k", str(case.k), "-b", str(case.b),
                        "-o", out, "-m", str(case.m), "-t", "4", "--abundance", str(case.a), "--noseq"], capture_output=True, text=True,
                       env=dict(os.environ, LCB_SEEDS="device", LCB_VERBOSE="1"))
    assert r.returncode == 0, r.stderr
    assert "lcb: device seeds=" in r.stderr
    assert open(os.path.join(out, "blocks_coords.gff")).read() == case.golden("ref.gff")
