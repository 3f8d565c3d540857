"""The capacity ladder on the device (run with -m gpu on an MI355X): the inputs of tests/ladder_inputs.py reach the pool limits of the kernel variants by
themselves, so the seeds climb compact -> wide -> big -> huge and double the huge workspace through the product's own host code (gatherBatch,
nextVariant, runToCompletion, allocWork in csrc/device.hip) - no variant is forced on a seed that would not have reached it and no pool is shrunk.
Every result is compared exactly with the CPU oracle on the same input; Device.mode_seeds() and Device.overflows() say which way the seeds went, and
the input's property is asserted on them first, so an input that drifts fails instead of passing below the limit it stands for.
(The result snapshot holds as many entries as the instance pool in every variant, so no seed leaves a variant because of it: not contrived here.)"""
import numpy as np
import pytest

import sibeliaz_amd
from tests import ladder_inputs as li
from tests.oracle_binding import Oracle, OrcCounters

pytestmark = pytest.mark.gpu

K, B, M, A = li.K, li.B, li.M, li.ABUNDANCE
N_LIGHT = 200           # light seeds (the tail of the seed order) placed behind the heavy ones of a tails input
_made = {}


def _tuples(inst):
    return [(int(a["chr"]), int(a["front_idx"]), int(a["back_idx"]), int(a["positive"]) != 0) for a in inst]


def _head_len(kind, params):
    return 16 if kind == "joiners" and params[0] >= 4000 else 300


@pytest.fixture(scope="module")
def ladder(built, tmp_path_factory):
    """(kind, params) -> the input, its storage, the seeds under test and the oracle's answers for them in the unused state and in the final `used`
    state of its own FindBlocks (with the event counters of either), computed once, shared by the tests and never changed."""
    tmp = tmp_path_factory.mktemp("gpu_ladder")

    def get(kind, params, final=True):
        key = (kind, params)
        if key not in _made:
            gr, fa = (li.joiners if kind == "joiners" else li.tails)(tmp, *params)
            st = sibeliaz_amd.JunctionStorage(gr, [fa], K, threads=4, abundance=A)
            seeds = st.seeds(4)
            li.check_property(kind, params, seeds)
            if kind == "joiners":
                head = seeds[:_head_len(kind, params)]
            else:           # the heaviest seeds, then seeds of few occurrences: a workgroup that wiped its vote table goes on to further seeds
                assert len(seeds) > li.HEAVY + N_LIGHT and int(seeds["count"][-N_LIGHT]) <= 4
                head = np.concatenate([seeds[:li.HEAVY], seeds[-N_LIGHT:]])
            _made[key] = dict(kind=kind, params=params, st=st, seeds=seeds, head=head, ref={}, ctr={}, orc=Oracle(gr, [fa], K, A), p=sibeliaz_amd.Params.make(K, b=B, m=M))
        x = _made[key]
        for state in ("unused", "final")[:2 if final else 1]:
            if state in x["ref"]:
                continue
            if state == "final":        # (the oracle's own FindBlocks leaves its `used` state behind: the unused answers are taken first)
                x["blocks"], x["stats"] = x["orc"].find_blocks(K, B, M)
                x["final"] = np.array(x["orc"].used_bitmap(x["st"].chr_start()), dtype="<u4")
            x["ctr"][state] = OrcCounters()
            x["ref"][state] = [x["orc"].process_seed(K, B, M, int(s["vid"]), int(s["ch"]), counters=x["ctr"][state]) for s in x["head"]]
            assert max(len(r[0]) for r in x["ref"][state]) < (1 << 16)       # (the oracle's result buffer)
        return x
    return get


def _process_once(dev, seeds, cap):
    """Device.process_seeds as ONE call of the library (the binding calls again with a larger buffer when the instances do not fit its first guess, which
    a test that counts launches and seeds per call cannot have): cap instances are known to do."""
    import ctypes as C
    s = np.ascontiguousarray(seeds, dtype=sibeliaz_amd.SEED_DTYPE)
    offsets, score, inst = np.zeros(len(s) + 1, dtype="<u8"), np.zeros(len(s), dtype="<i8"), np.zeros(cap, dtype=sibeliaz_amd.INSTANCE_DTYPE)
    ctr = sibeliaz_amd.api.Counters()
    rc = dev.L.lcb_process_seeds(dev.h, s.ctypes.data, len(s), offsets.ctypes.data, inst.ctypes.data, cap, score.ctypes.data, C.byref(ctr))
    assert rc == 0, dev.L.lcb_last_error()
    return offsets, inst[: int(offsets[len(s)])], score, ctr.as_dict()


def _compare(x, dev, state, what, once=False, first=None):
    seeds, ref = x["head"][:first], x["ref"][state][:first]
    off, inst, score, ctr = _process_once(dev, seeds, sum(len(r[0]) for r in ref) + 64) if once else dev.process_seeds(seeds, counters=True)
    bad = [i for i, (r, r_score) in enumerate(ref) if _tuples(inst[int(off[i]):int(off[i + 1])]) != r or int(score[i]) != r_score]
    assert not bad, "%s%r, %s, %s state: %d of %d seeds differ from the oracle, first %s (vid %d)" % (x["kind"], x["params"], what, state, len(bad), len(seeds), bad[:5],
                                                                                                    int(seeds["vid"][bad[0]]))
    return off, inst, score, ctr


@pytest.mark.parametrize("pools", [1, 2])
@pytest.mark.parametrize("params", [(120, 10, 5, 3), (250, 10, 5, 3), (1000, 30, 5, 3), (4090, 10, 5, 3)])
def test_climb_from_the_compact_variant(ladder, params, pools):
    """Every seed starts in the compact variant with either pool size; the heaviest outgrow the instance pool of every variant the input's property
    names (in the path's initialisation, or in the push that reaches R2) and end where it says: wide for 130 and 260 occurrences, big for 1 030, the
    doubled huge workspace for 4 100. Then the same seeds in the oracle's final `used` state."""
    x = ladder("joiners", params)
    dev = sibeliaz_amd.Device(x["st"], x["p"], 0, start_mode=1, compact_pools=pools)
    try:
        _compare(x, dev, "unused", "compact pools %d" % pools)
        counts, ov = dev.mode_seeds(), dev.overflows()
        print("joiners%r pools %d: mode_seeds %s overflows %s" % (params, pools, counts, ov))
        li.check_property("joiners", params, x["seeds"], li.device_exits(ov), pools=pools)
        left = li.JOINERS[params][pools]
        assert counts[0] >= len(x["head"]), counts
        for i, v in enumerate(li.VARIANTS[1:], 1):
            assert (counts[i] > 0) == (li.VARIANTS[i - 1] in left), (v, counts)
        assert ov["huge_inst_cap"] >= li.HUGE_IC << li.JOINERS[params]["grow"], ov
        dev.set_used(x["final"])
        _compare(x, dev, "final", "compact pools %d" % pools)
    finally:
        dev.close()


@pytest.mark.parametrize("pools", [1, 2])
@pytest.mark.parametrize("params", list(li.TAILS))
def test_vote_table_exits(ladder, params, pools):
    """The vote table fills while the instance pool is within its limits - out of compact (both pools), wide and big in turn by the input - and the
    seed runs again in the next variant: first the heaviest seeds alone, whose exits are vote-table exits only. Then with 200 seeds of few occurrences
    behind them and few workgroups per variant: a workgroup that wiped its table after the overflow goes on to further seeds, which must be right as
    well. (A seed of two occurrences in a tail reaches R and its pool: those seeds climb too, by either limit.)"""
    x = ladder("tails", params)
    dev = sibeliaz_amd.Device(x["st"], x["p"], 0, start_mode=1, compact_pools=pools, compact_slots=4, wide_slots=2, big_slots=4, huge_slots=4)
    try:
        _compare(x, dev, "unused", "the heaviest alone, compact pools %d" % pools, first=li.HEAVY)
        ov = dev.overflows()
        print("tails%r pools %d, the heaviest %d: mode_seeds %s overflows %s" % (params, pools, li.HEAVY, dev.mode_seeds(), ov["counts"]))
        li.check_property("tails", params, x["seeds"], li.device_exits(ov), pools=pools, heavy_only=True)
        _compare(x, dev, "unused", "compact pools %d" % pools)
        ov = dev.overflows()
        print("tails%r pools %d: mode_seeds %s overflows %s" % (params, pools, dev.mode_seeds(), ov))
        li.check_property("tails", params, x["seeds"], li.device_exits(ov), pools=pools)
        assert ov["huge_inst_cap"] == li.HUGE_IC
        dev.set_used(x["final"])
        _compare(x, dev, "final", "compact pools %d" % pools)
    finally:
        dev.close()
    # whether a seed leaves a variant does not depend on what its workgroup ran before: with the default slots (a workgroup per seed here)
    # the same calls count the same exits
    dev = sibeliaz_amd.Device(x["st"], x["p"], 0, start_mode=1, compact_pools=pools)
    try:
        _compare(x, dev, "unused", "the heaviest alone, default slots", first=li.HEAVY)
        _compare(x, dev, "unused", "default slots")
        assert dev.overflows()["counts"] == ov["counts"], (dev.overflows()["counts"], ov["counts"])
    finally:
        dev.close()


@pytest.mark.parametrize("params,factor", [((4090, 10, 5, 3), 2), ((8190, 5, 5, 3), 4), (li.SNAPSHOT_EDGE, 4)])
def test_huge_workspace_grows(ladder, params, factor, tmp_path, monkeypatch):
    """A default device: the heaviest 16 seeds climb from the wide variant into the huge one, whose workspace doubles until they fit (the pool of
    such a seed reaches about twice its occurrences: at least x2 for 4 100, x4 for 8 195) - one huge launch more than doublings, the oracle's
    results. A second identical call gives the same bytes, starts every seed where the hints say (nothing in the compact variant, nothing in the
    wide one that left it before) and grows nothing. Then the footprints out of the regrown workspace cover every read."""
    x = ladder("joiners", params, final=False)
    trace = tmp_path / "launches.tsv"
    monkeypatch.setenv("LCB_TRACE_LAUNCHES", str(trace))
    dev = sibeliaz_amd.Device(x["st"], x["p"], 0)
    try:
        head, n = x["head"], len(x["head"])
        off, inst, score, _ = _compare(x, dev, "unused", "default device", once=True)
        if params == li.SNAPSHOT_EDGE:      # (results that only a snapshot buffer doubled with the pool can hold)
            assert max(int(off[i + 1] - off[i]) for i in range(n)) > li.HUGE_IC
        c1, ov1 = dev.mode_seeds(), dev.overflows()
        grown = ov1["huge_inst_cap"] // li.HUGE_IC
        print("joiners%r: huge workspace x%d (%d instances), mode_seeds %s, overflows %s" % (params, grown, ov1["huge_inst_cap"], c1, ov1["counts"]))
        li.check_property("joiners", params, x["seeds"], li.device_exits(ov1), start="wide")       # (a call of 16 seeds begins in the wide variant)
        first_launches = dev.kernel_time()[1]
        assert grown >= factor and grown & (grown - 1) == 0, ov1
        off2, inst2, score2, _ = _process_once(dev, head, len(inst) + 64)
        c2, ov2 = dev.mode_seeds(), dev.overflows()
        assert off2.tobytes() == off.tobytes() and inst2.tobytes() == inst.tobytes() and score2.tobytes() == score.tobytes()
        to_big, to_huge = sum(ov1["counts"]["wide"].values()), sum(ov1["counts"]["big"].values())
        delta = [b - a for a, b in zip(c1, c2)]
        print("second call: mode_seeds +%s" % (delta,))
        assert delta[0] == 0 and delta[3] == to_huge and delta[1] + delta[2] == n - to_huge and delta[1] <= n - to_big, (delta, c1, ov1)
        assert ov2 == ov1, (ov1, ov2)
        # the footprint slots of the regrown workspace: with every unused position outside a seed's footprint set to used, the seed gives the same result
        off3, inst3, fp_off, fp = dev.process_seeds_fp(head)
        assert inst3.tobytes() == inst.tobytes()
        assert dev.overflows()["huge_inst_cap"] == ov1["huge_inst_cap"]
        picked = [i for i in range(n) if off[i + 1] - off[i] > 1][:8]
        assert picked, "no heavy seed yields a block"
        words = (x["st"].n_positions() + 31) // 32 + 1
        for i in picked:
            bits = np.ones(words * 32, dtype=bool)
            for lo, hi in fp[int(fp_off[i]):int(fp_off[i + 1])]:
                bits[int(lo):int(hi) + 1] = False
            dev.set_used(np.packbits(bits, bitorder="little").view("<u4"))
            _, inst4, _, _ = dev.process_seeds_fp(head[i:i + 1])
            assert inst4.tobytes() == inst[int(off[i]):int(off[i + 1])].tobytes(), "seed %d: a read outside its footprint changed the result" % i
    finally:
        dev.close()
    log2 = grown.bit_length() - 1
    first_call = [ln.split("\t") for ln in trace.read_text().splitlines() if not ln.startswith("#")][:first_launches]
    assert len(first_call) == first_launches and sum(1 for r in first_call if r[3] == "huge") == log2 + 1, [(r[1], r[3]) for r in first_call]


@pytest.mark.parametrize("mode", [2, 3, 4])
@pytest.mark.parametrize("kind,params", [("joiners", (1000, 30, 5, 3)), ("tails", (500, 4, 20, 5))])
def test_started_in_each_16_wavefront_variant(ladder, kind, params, mode):
    """Every seed started in the wide, big and huge variant: votes of about 1 000 voters, above LCB_VOTE_RESOLVE_MAX. Both `used` states; with the
    stats kernels the summed event counters are the oracle's."""
    x = ladder(kind, params)
    dev = sibeliaz_amd.Device(x["st"], x["p"], 0, start_mode=mode)
    try:
        for state in ("unused", "final"):
            if state == "final":
                dev.set_used(x["final"])
            _compare(x, dev, state, "start_mode %d" % mode)
        counts = dev.mode_seeds()
        assert counts[mode - 1] >= 2 * len(x["head"]) and all(c == 0 for c in counts[:mode - 1]), counts
        dev.set_stats_mode(True)
        for state in ("final", "unused"):
            if state == "unused":
                dev.reset_used()
            _, _, _, ctr = _compare(x, dev, state, "start_mode %d, stats" % mode)
            assert ctr == x["ctr"][state].as_dict(), state
    finally:
        dev.close()


@pytest.mark.parametrize("kind,params", [("joiners", (1000, 30, 5, 3)), ("tails", (500, 4, 20, 5))])
def test_whole_pass(ladder, kind, params):
    """FindBlocks on a default device (side lanes on: a heavy job on a lane ends in the big variant or with a hint for it), and with the lanes off:
    the oracle's blocks, blocks found and failures; a second pass on the same device gives the same bytes."""
    x = ladder(kind, params)
    ref = x["blocks"]
    for knobs in ({}, {"sync_jobs": 1}):
        dev = sibeliaz_amd.Device(x["st"], x["p"], 0)
        try:
            finder = sibeliaz_amd.BlocksFinder(x["st"], K)
            blocks = finder.FindBlocks(M, B, device=dev, seeds=x["seeds"], threads=4, **knobs).copy()
            stats = dict(finder.stats)
            blocks2 = finder.FindBlocks(M, B, device=dev, seeds=x["seeds"], threads=4, **knobs)
            counts, ov = dev.mode_seeds(), dev.overflows()["counts"]
            print("%s%r %s: mode_seeds %s overflows %s side lanes: %s" % (kind, params, knobs, counts, ov, {k: v for k, v in stats.items() if k.startswith("side_")}))
            # the pass really climbed: seeds left the wide variant for the big one. With the lanes on, background batches ran and their results were
            # used; on the joiners input jobs that outgrew their variant on a lane came back without a result (the hint branch of the lane's poll) -
            # the jobs of the tails input that leave the wide variant there are re-run by the lane itself in its big variant and come back with one.
            assert counts[2] > 0 and sum(ov["wide"].values()) > 0, (counts, ov)
            if knobs:
                assert stats["side_batches"] == 0, stats
            else:
                assert stats["side_batches"] > 0 and stats["side_taken"] > 0 and (stats["side_failed"] > 0 or kind == "tails"), stats
            assert len(blocks) == len(ref), (len(blocks), len(ref))
            for f in ("id", "chr", "start", "end"):
                assert np.array_equal(np.asarray(blocks[f], dtype=np.int64), np.asarray(ref[f], dtype=np.int64)), f
            assert stats["blocks_found"] == x["stats"]["blocks_found"] and stats["failures"] == x["stats"]["failures"]
            assert blocks.tobytes() == blocks2.tobytes()
        finally:
            dev.close()


def test_the_claim_limit_is_three_quarters_of_the_table(built, tmp_path):
    """A vote of exactly 385 distinct candidates overflows the 512-slot table of the small compact pools (384 may be claimed): of the first 150 seeds of
    ladder_inputs.CLAIM_EDGE exactly 26 leave the compact variant, all because of the vote table - the emulator's count. The oracle's results."""
    params, seed, n, want = li.CLAIM_EDGE
    gr, fa = li.tails(tmp_path, *params, seed=seed)
    st = sibeliaz_amd.JunctionStorage(gr, [fa], K, threads=4, abundance=A)
    seeds = st.seeds(4)[:n]
    orc = Oracle(gr, [fa], K, A)
    x = dict(kind="tails", params=params, head=seeds, ref={"unused": [orc.process_seed(K, B, M, int(s["vid"]), int(s["ch"])) for s in seeds]})
    dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(K, b=B, m=M), 0, start_mode=1, compact_pools=2)
    try:
        _compare(x, dev, "unused", "small compact pools", once=True)
        counts, ov = dev.mode_seeds(), dev.overflows()["counts"]
        print("claim edge: mode_seeds %s overflows %s" % (counts, ov))
        assert ov["compact"] == dict(instances=0, vote=want, path=0, snapshot=0) and counts == (n, want, 0, 0), (counts, ov)
    finally:
        dev.close()


def test_a_full_path_set_chooses_the_variant_by_the_instances(ladder):
    """The one place where the ladder is no ladder (nextVariant): a seed that fills the wide variant's LDS path set goes back to the compact variant
    (path set in HBM) if it holds few instances, and on to the big one if it holds more than half the compact pool - where the seeds of 130
    occurrences of joiners(120, 10) belong. A 16-vertex wide path set makes every longer path take that decision; the oracle's results."""
    x = ladder("joiners", (120, 10, 5, 3))
    dev = sibeliaz_amd.Device(x["st"], x["p"], 0, start_mode=2, wide_path_cap=16)
    try:
        _compare(x, dev, "unused", "wide path set of 16")
        counts, ov = dev.mode_seeds(), dev.overflows()
        print("wide path set of 16: mode_seeds %s overflows %s" % (counts, ov["counts"]))
        assert ov["counts"]["wide"]["path"] > 0 and counts[0] > 0 and counts[2] > 0 and counts[0] + counts[2] >= ov["counts"]["wide"]["path"], (counts, ov)
        assert counts[3] == 0 and sum(ov["counts"]["big"].values()) == 0, (counts, ov)
    finally:
        dev.close()


def test_segments(ladder):
    """joiners(1000, 30) in several segments (seg_cap: a record each), every seed from the compact variant up: the segment-aware kernels of the
    variants up to big, where a footprint slot that instances of two segments would share also ends the seed with the instance-pool status."""
    x = ladder("joiners", (1000, 30, 5, 3))
    cs = x["st"].chr_start()
    cap = int(max(cs[1:] - cs[:-1])) + 8
    assert len(cs) - 1 >= 5 and int(cs[-1]) > 3 * cap
    dev = sibeliaz_amd.Device(x["st"], x["p"], 0, start_mode=1, seg_cap=cap)
    try:
        _compare(x, dev, "unused", "segments")
        counts, ov = dev.mode_seeds(), dev.overflows()
        print("segments of at most %d positions: mode_seeds %s overflows %s" % (cap, counts, ov["counts"]))
        li.check_property("joiners", x["params"], x["seeds"], li.device_exits(ov), segmented=True)
        assert counts[2] > 0
        dev.set_used(x["final"])
        _compare(x, dev, "final", "segments")
    finally:
        dev.close()
