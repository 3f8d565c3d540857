"""The capacity ladder at its real pool boundaries, under the wavefront emulator (CPU): seeds that outgrow a kernel variant's instance pool or vote
table by themselves - no forced variant, no shrunk pool - run again in the next variant, compact -> wide -> big -> huge, and in the huge variant
again after its workspace has doubled. Inputs: tests/ladder_inputs.py. Every run compares each seed with the CPU oracle (and, in the stats flavour,
the event counters); the emulator's `ladder:` lines say which variant the seeds left and why, and the input's property is asserted on them, so an
input that drifts fails here instead of passing without reaching the limit it stands for.

Two flavours: the instrumented kernels with one wavefront (event counters equal the oracle's), and the shipped ones (EMU_NOSTATS=1) with the product's
wavefront count in every variant (EMU_NW=2 for the compact one, EMU_RETRY_NW=shipped for the retries: 16 / 16 / 8), with the footprint-completeness
check at the smaller sizes."""
import os
import subprocess

import pytest

import sibeliaz_amd
from tests import ladder_inputs as li

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "build", "emu_check")

STATS = {}
SHIPPED = {"EMU_NOSTATS": "1", "EMU_NW": "2", "EMU_RETRY_NW": "shipped"}
SHIPPED_FP = dict(SHIPPED, EMU_FP_CHECK="1")
SHIPPED_NW = (2, 16, 16, 8)      # compact / wide / big / huge: LCB_NW_COMPACT, LCB_NW_WIDE, LCB_NW_BIG, LCB_NW_HUGE of csrc/device.hip


@pytest.fixture(scope="module")
def emu_built(built):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """(kind, params) -> (graph, fasta, the host enumerator's seeds), generated once."""
    tmp = tmp_path_factory.mktemp("ladder")
    made = {}

    def get(kind, params):
        if (kind, params) not in made:
            gr, fa = (li.joiners if kind == "joiners" else li.tails)(tmp, *params)
            st = sibeliaz_amd.JunctionStorage(gr, [fa], li.K, threads=2, abundance=li.ABUNDANCE)
            made[(kind, params)] = (gr, fa, st.seeds(2))
        return made[(kind, params)]
    return get


def _run(gr, fa, mode, limit, env):
    r = subprocess.run([EMU, gr, fa, str(li.K), str(li.B), str(li.M), str(li.ABUNDANCE), mode], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, EMU_LIMIT=str(limit), **env))
    ladder = [ln for ln in r.stderr.splitlines() if ln.startswith("ladder:")]
    print("\n".join(ladder))
    assert r.returncode == 0 and "FAIL" not in r.stderr and "MISMATCH" not in r.stderr and ", 0 mismatches" in r.stderr, r.stderr[-1500:]
    exits, grown = li.parse_ladder(r.stderr)
    # no silent fall-back: the shipped flavour ran every variant it visited with the product's wavefront count, the stats flavour with one
    first = {"seeds-init": 0, "seeds-final": 0, "medium": 1, "big": 2, "huge": 3}[mode]
    for i, v in enumerate(li.VARIANTS):
        want = (int(env["EMU_NW"]) if i == first else SHIPPED_NW[i]) if env.get("EMU_NOSTATS") else 1
        assert exits[v]["nw"] <= {want}, "%s ran with %s wavefronts, %d expected" % (v, sorted(exits[v]["nw"]), want)
    return exits, grown


def _limit(params):
    return 12 if params[0] >= 4000 else (100 if params[0] >= 1000 else 200)


@pytest.mark.parametrize("flavour", ["stats", "shipped"])
@pytest.mark.parametrize("params", [p for p in li.JOINERS if p != li.SNAPSHOT_EDGE])
def test_joiners_climb_by_the_instance_pool(emu_built, inputs, params, flavour):
    """Seeds of n1 + n2 occurrences fill the instance pool when the path is initialised, seeds of n1 when a push reaches R2: they leave every variant
    whose pool they outgrow, end where the input's property says, and at the two largest sizes only after the huge workspace has doubled (once for
    4 100 occurrences, twice for 8 195). Then the same seeds in the oracle's final `used` state."""
    gr, fa, seeds = inputs("joiners", params)
    li.check_property("joiners", params, seeds)
    env = STATS if flavour == "stats" else (SHIPPED_FP if params[0] <= 1000 else SHIPPED)
    exits, grown = _run(gr, fa, "seeds-init", _limit(params), env)
    li.check_property("joiners", params, seeds, exits, grown)
    assert grown == [li.HUGE_IC << (i + 1) for i in range(len(grown))], grown
    _run(gr, fa, "seeds-final", _limit(params), env)


@pytest.mark.parametrize("flavour", ["stats", "shipped"])
@pytest.mark.parametrize("params", [(120, 10, 5, 3), (250, 10, 5, 3)])
def test_joiners_small_compact_pools(emu_built, inputs, params, flavour):
    """The 128-instance pools of the compact variant (EMU_COMPACT_SMALL): 130 occurrences are two more than the pool holds."""
    gr, fa, seeds = inputs("joiners", params)
    li.check_property("joiners", params, seeds)
    env = dict(STATS if flavour == "stats" else SHIPPED_FP, EMU_COMPACT_SMALL="1")
    exits, grown = _run(gr, fa, "seeds-init", 200, env)
    li.check_property("joiners", params, seeds, exits, grown, pools=2)
    _run(gr, fa, "seeds-final", 200, env)


@pytest.mark.parametrize("flavour", ["stats", "shipped"])
@pytest.mark.parametrize("pools", [1, 2])
@pytest.mark.parametrize("params", list(li.TAILS))
def test_tails_climb_by_the_vote_table(emu_built, inputs, params, pools, flavour):
    """Few instances, many distinct candidates per voter: the vote table fills (three quarters of its slots claimed) while the pool is within its
    limits, the table is wiped and the seed runs again in the next variant - out of compact (both pools), wide and big in turn. The heavy head of
    the seed order for the results, its first HEAVY seeds alone for the exits that must be vote-table exits only."""
    gr, fa, seeds = inputs("tails", params)
    li.check_property("tails", params, seeds)
    env = dict(STATS if flavour == "stats" else SHIPPED_FP)
    if pools == 2:
        env["EMU_COMPACT_SMALL"] = "1"
    head = 100 if params[0] <= 100 else 40
    exits, grown = _run(gr, fa, "seeds-init", head, dict(env, EMU_THREADS="4"))
    li.check_property("tails", params, seeds, exits, grown, pools=pools)
    # whether a seed leaves a variant does not depend on what its workgroup ran before: one emulated workgroup for all the seeds, one after the
    # other (the table wiped after every overflow), sees the exits that four see
    if params[0] <= 100:         # (the two inputs whose heads hold seeds that stay in the compact variant behind seeds that leave it; the larger ones only cost time)
        serial, _ = _run(gr, fa, "seeds-init", 100, dict(env, EMU_THREADS="1"))
        assert serial == exits, (serial, exits)
    exits, grown = _run(gr, fa, "seeds-init", li.HEAVY, env)
    li.check_property("tails", params, seeds, exits, grown, pools=pools, heavy_only=True)
    assert not grown
    _run(gr, fa, "seeds-final", head, env)


def _segments(gr, fa, env):
    r = subprocess.run([EMU, gr, fa, str(li.K), str(li.B), str(li.M), str(li.ABUNDANCE), "seeds-init"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, EMU_LIMIT="1", EMU_SEG_VERBOSE="1", **env))
    n_seg = [int(ln.split()[1]) for ln in r.stderr.splitlines() if ln.startswith("emu:") and "segments over" in ln]
    assert n_seg, r.stderr[-800:]
    return n_seg[0]


@pytest.mark.parametrize("flavour", ["stats", "shipped"])
@pytest.mark.parametrize("params,seg_cap,ends", [((1000, 30, 5, 3), 3000, "big"), ((4090, 10, 5, 3), 14000, "huge")])
def test_joiners_in_segments(emu_built, inputs, params, seg_cap, ends, flavour):
    """The inputs cut into five segments, a record each (EMU_SEG_CAP): the segment-aware instantiations of every variant, with seeds that end in the big
    variant (1 030 occurrences) and in the huge one after its workspace has doubled (4 100)."""
    gr, fa, seeds = inputs("joiners", params)
    li.check_property("joiners", params, seeds)
    env = dict(STATS if flavour == "stats" else (SHIPPED_FP if params[0] <= 1000 else SHIPPED), EMU_SEG_CAP=str(seg_cap))
    assert _segments(gr, fa, env) == 5
    exits, grown = _run(gr, fa, "seeds-init", _limit(params), env)
    li.check_property("joiners", params, seeds, exits, grown, segmented=True)
    assert exits[ends]["ok"] > 0 and all(exits[v]["ok"] == 0 for v in li.VARIANTS[li.VARIANTS.index(ends) + 1:]), exits
    if ends == "huge":
        # the other way to the instance-pool status, in lcb_push: a new instance of the backward extension finds no footprint slot of its own left and the
        # one it would share belongs to another segment. Some of the seeds leave the 8 192-instance workspace that way, with the pool not full (`clash`).
        assert exits["huge"]["clash"] > 0 and exits["huge"]["inst"] > exits["huge"]["clash"], exits
    _run(gr, fa, "seeds-final", _limit(params), env)


@pytest.mark.parametrize("flavour", ["stats", "shipped"])
def test_the_claim_limit_is_three_quarters_of_the_table(emu_built, tmp_path, flavour):
    """A vote of exactly 385 distinct candidates overflows the 512-slot table (384 may be claimed): ladder_inputs.CLAIM_EDGE."""
    params, seed, n, want = li.CLAIM_EDGE
    gr, fa = li.tails(tmp_path, *params, seed=seed)
    exits, _ = _run(gr, fa, "seeds-init", n, dict(STATS if flavour == "stats" else SHIPPED_FP, EMU_COMPACT_SMALL="1"))
    assert exits["compact"]["vote"] == want and exits["compact"]["inst"] == 0 and exits["compact"]["ok"] == n - want, exits
    assert exits["wide"]["ok"] == want, exits


@pytest.mark.parametrize("cap,mode", [(1024, "medium"), (4096, "big")])
def test_a_pool_holds_exactly_its_capacity(emu_built, tmp_path, cap, mode):
    """The comparison itself: seed_inputs.heavy without reverse complements has ONE seed of n occurrences, whose pool stays at n in these two variants.
    With n = the variant's pool it does not leave because of the pool (the wide variant keeps it; the big one loses it to its vote table), with
    n = pool + 1 it does, in the path's initialisation. The seed is started in the variant (`medium`, `big`)."""
    from tests import seed_inputs as si
    for n, leaves in ((cap, 0), (cap + 1, 1)):
        gr, fa = si.heavy(tmp_path, n, 5, 10 * n, 0)
        seeds = sibeliaz_amd.JunctionStorage(gr, [fa], li.K, threads=2, abundance=li.ABUNDANCE).seeds(2)
        assert int(seeds["count"][0]) == n and int(seeds["count"][1]) < n
        for env in (STATS, dict(SHIPPED, EMU_NW="16")):        # (16 wavefronts: what the product launches either variant with)
            exits, _ = _run(gr, fa, mode, 1, env)
            v = li.VARIANTS[1 if mode == "medium" else 2]
            assert exits[v]["inst"] == leaves and exits[v]["ok"] + exits[v]["vote"] == 1 - leaves, (n, exits)


def test_small_huge_workspace_grows_on_a_small_input(emu_built, inputs):
    """EMU_HUGE_CAP=256: the huge variant starts with 256 instances and a vote table of 2 048 slots; the heaviest seeds of joiners(4090, 10) double
    it from there to 16 384 - six growths, each laying the slot out and initialising it again."""
    params = (4090, 10, 5, 3)
    gr, fa, seeds = inputs("joiners", params)
    li.check_property("joiners", params, seeds)
    exits, grown = _run(gr, fa, "seeds-init", 4, dict(SHIPPED, EMU_HUGE_CAP="256"))
    assert grown[:6] == [512, 1024, 2048, 4096, 8192, 16384], grown
    assert exits["huge"]["inst"] + exits["huge"]["vote"] >= 6, exits
