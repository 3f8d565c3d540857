"""GPU tests (-m gpu) on the full-size draws of the randomized campaign (tests/fuzz_inputs.py; tests/emu/fuzz.py draws them, the
emulator campaign runs their small siblings): every k, b and m of the campaign and all three abundance limits, N runs, tandem repeats,
inversions, several chromosomes, up to 20 strains - inputs the goldens do not contain, on the hardware the emulator stands in for (DPP
ladders, voter tickets, LDS vote-table inserts, the barriers between seed wave and helper waves, the STATS instantiations). Everything
is compared with the CPU oracle, exactly: per-seed results of each kernel variant in three `used` states, both pool sizes of the compact
variant, the event counters, whole FindBlocks runs with the draw's engine knobs, segmented device tables, the routes that build on the
device. tests/test_fuzz_inputs_cpu.py checks that the draws and the sampled seeds have something to compare. The oracle's answers are
computed once per (draw, state, seed) and shared."""
import numpy as np
import pytest

import sibeliaz_amd
from tests import fuzz_inputs
from tests.fuzz_inputs import DRAWS
from tests.test_gpu_handover import _check, _done
from tests.test_gpu_parity import _compare_results
from tests.test_gpu_segments import _seg_setup
from tests.test_gpu_tables import _same_tables

pytestmark = pytest.mark.gpu

SEGMENT_DRAWS = [9, 20, 34]


@pytest.fixture(scope="module")
def pool(built, tmp_path_factory):
    return fuzz_inputs.DrawPool(tmp_path_factory.mktemp("gpu_fuzz"))


def _indices(d, mode):
    if mode == 1:
        return np.arange(len(d.seeds))
    return fuzz_inputs.sample(d.seeds, *(fuzz_inputs.SAMPLE_HUGE if mode == 4 else fuzz_inputs.SAMPLE_16))


def _parity(d, dev, idx, state, what):
    """seeds[idx] on `dev` in `state` against the oracle's answers."""
    dev.set_used(d.states[state])
    seeds = d.seeds[idx]
    _compare_results(dev.process_seeds(seeds), seeds, d.refs(state, idx), "draw %d, %s, %s state" % (d.draw, what, state))


@pytest.mark.parametrize("state", fuzz_inputs.STATES)
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("draw", DRAWS)
def test_per_seed_parity(pool, draw, mode, state):
    """ProcessVertex::Process of one kernel variant (1 compact, 2 wide, 3 big, 4 huge) against the oracle: every seed in the compact
    variant, the heavy head of the seed order and a stride through the rest in the others; the seeds ran where they were sent."""
    d = pool.get(draw)
    idx = _indices(d, mode)
    dev = sibeliaz_amd.Device(d.st, sibeliaz_amd.Params.make(d.k, b=d.b, m=d.m), 0, start_mode=mode)
    try:
        _parity(d, dev, idx, state, "variant %d" % mode)
        counts = dev.mode_seeds()
    finally:
        dev.close()
    assert counts[mode - 1] >= len(idx) and all(c == 0 for c in counts[:mode - 1]), counts


@pytest.mark.parametrize("pools", [1, 2])
@pytest.mark.parametrize("draw", DRAWS)
def test_compact_pools(pool, draw, pools):
    """Every seed started in the compact variant with either of its pool sizes (1 = 256 instances / 1 024 vote slots, 2 = 128 / 512); the
    seeds that outgrow the pools go up the ladder - draw 20 has a seed of 131 instances - and the results stay the oracle's."""
    d = pool.get(draw)
    idx = _indices(d, 1)
    dev = sibeliaz_amd.Device(d.st, sibeliaz_amd.Params.make(d.k, b=d.b, m=d.m), 0, start_mode=1, compact_pools=pools)
    try:
        _parity(d, dev, idx, "unused", "compact pools %d" % pools)
        counts = dev.mode_seeds()
    finally:
        dev.close()
    assert counts[0] >= len(idx), counts
    if draw == 20 and pools == fuzz_inputs.COMPACT_POOLS_SMALL:
        assert sum(counts[1:]) > 0, counts


@pytest.mark.parametrize("draw", DRAWS)
def test_event_counters(pool, draw):
    """The STATS instantiations of the kernels: the event counters of every seed, summed, are the oracle's."""
    d = pool.get(draw)
    dev = sibeliaz_amd.Device(d.st, sibeliaz_amd.Params.make(d.k, b=d.b, m=d.m), 0)
    try:
        dev.set_stats_mode(True)
        results = dev.process_seeds(d.seeds, counters=True)
    finally:
        dev.close()
    assert results[3] == d.counters()
    _compare_results(results, d.seeds, d.refs("unused", range(len(d.seeds))), "draw %d, stats kernels" % draw)


def _find_blocks(d, knobs, opts, what):
    ref, ref_stats = d.blocks()
    dev = sibeliaz_amd.Device(d.st, sibeliaz_amd.Params.make(d.k, b=d.b, m=d.m), 0, **opts)
    try:
        finder = sibeliaz_amd.BlocksFinder(d.st, d.k)
        blocks = finder.FindBlocks(d.m, d.b, device=dev, seeds=d.seeds, threads=4, **knobs).copy()
        stats = dict(finder.stats)
        again = finder.FindBlocks(d.m, d.b, device=dev, seeds=d.seeds, threads=4, **knobs)
        same = blocks.tobytes() == again.tobytes()
    finally:
        dev.close()
    assert len(blocks) == len(ref), "draw %d, %s: %d blocks, the oracle has %d" % (d.draw, what, len(blocks), len(ref))
    for f in ("id", "chr", "start", "end"):
        assert np.array_equal(np.asarray(blocks[f], dtype=np.int64), np.asarray(ref[f], dtype=np.int64)), "draw %d, %s: %s" % (d.draw, what, f)
    assert stats["blocks_found"] == ref_stats["blocks_found"] and stats["failures"] == ref_stats["failures"], (what, stats, ref_stats)
    assert same, "draw %d, %s: a second pass on the same device gives other bytes" % (d.draw, what)


@pytest.mark.parametrize("draw", DRAWS)
def test_find_blocks(pool, draw):
    """Whole FindBlocks runs against the oracle's: default knobs, the knobs of the draw's first `find` run of the campaign, and the side
    lanes of its side-lane run with a tiny job cap; each with a second pass on the same device."""
    d = pool.get(draw)
    (knobs, opts), (side_knobs, side_opts) = fuzz_inputs.find_knobs(draw)
    _find_blocks(d, {}, {}, "default knobs")
    _find_blocks(d, knobs, opts, "%r %r" % (knobs, opts))
    _find_blocks(d, side_knobs, side_opts, "%r %r" % (side_knobs, side_opts))


def _segments(d, flavour):
    idx = _indices(d, 2)
    for mode in (1, 2):
        st, p, dev = _seg_setup(d, flavour, start_mode=mode)
        try:
            assert st.seeds(4).tobytes() == d.seeds.tobytes()
            assert (dev.read_table("seg_base") != 0).any(), "one segment only"
            _parity(d, dev, idx, "random", "segments (%s), variant %d" % (flavour, mode))
            counts = dev.mode_seeds()
        finally:
            dev.close()
            st.close()
        assert counts[mode - 1] >= len(idx) and all(c == 0 for c in counts[:mode - 1]), counts


@pytest.mark.parametrize("flavour", ["many", "gap"])
@pytest.mark.parametrize("draw", SEGMENT_DRAWS)
def test_segments(pool, draw, flavour):
    """Positions as (segment, offset) pairs - the SEG instantiations - in the random `used` state (set_used lays the bitmap out segment
    by segment): a segment per chromosome or two, and a few segments with an odd gap between them; compact and wide variant."""
    _segments(pool.get(draw), flavour)


def test_segments_with_flat_indices_beyond_32_bits(pool):
    """The same with the second segment of draw 34 beyond 2^32 (about 43 GB of device tables)."""
    _segments(pool.get(34), "wide")


@pytest.mark.parametrize("draw", DRAWS)
def test_device_routes(pool, draw):
    """The routes that build on the device give what the file route gives (lcb-mkgraph, JunctionStorage, host tables, the host's seed
    enumeration): open_fasta - graph built on the device and handed over -, Device(tables="device") and enumerate_seeds()."""
    d = pool.get(draw)
    st, dev, stats, yst = _check(d.graph, [d.fasta], d.k, d.a, d.name, b=d.b, m=d.m)
    try:
        assert st.seeds(4).tobytes() == d.seeds.tobytes()
    finally:
        _done(st, dev)
    p = sibeliaz_amd.Params.make(d.k, b=d.b, m=d.m)
    host, tdev = sibeliaz_amd.Device(d.st, p, 0), sibeliaz_amd.Device(d.st, p, 0, tables="device")
    try:
        _same_tables(host, tdev, d.name)
        assert tdev.enumerate_seeds().tobytes() == d.seeds.tobytes() and host.enumerate_seeds().tobytes() == d.seeds.tobytes()
        idx = fuzz_inputs.sample(d.seeds, 100, 50)
        _parity(d, tdev, idx, "random", "device-built tables")
    finally:
        host.close()
        tdev.close()
