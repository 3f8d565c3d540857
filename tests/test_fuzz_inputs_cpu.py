"""The full-size draws of the randomized campaign that tests/test_gpu_fuzz.py runs on the device (tests/fuzz_inputs.py), checked with the
oracle alone: the conditions without which the device tests would pass vacuously - the inputs are the ones measured, their sampled
seeds do real work, the `random` state changes results - and the oracle's set_used, which puts it into that state."""
import numpy as np
import pytest

from tests import fuzz_inputs


@pytest.fixture(scope="module")
def pool(built, tmp_path_factory):
    return fuzz_inputs.DrawPool(tmp_path_factory.mktemp("fuzz_inputs"))


def test_sample_takes_the_head_and_strides_the_rest():
    assert list(fuzz_inputs.sample(range(7), 300, 100)) == list(range(7))
    assert list(fuzz_inputs.sample(range(300), 300, 100)) == list(range(300))
    s = fuzz_inputs.sample(range(1343), 300, 100)          # 1043 left: every 11th
    assert list(s[:300]) == list(range(300)) and list(s[300:]) == list(range(300, 1343, 11)) and len(s) == 395
    assert list(fuzz_inputs.sample(range(20), 4, 8)) == [0, 1, 2, 3] + list(range(4, 20, 2))


def test_draws_cover_the_campaigns_parameters():
    p = [fuzz_inputs.TABLE[d][0] for d in fuzz_inputs.DRAWS]
    assert [fuzz_inputs.fuzz.case_params(d, small=False)[1] for d in fuzz_inputs.DRAWS] == p
    assert {x[0] for x in p} == {11, 15, 21, 25} and {x[1] for x in p} == {40, 100, 200, 400} and {x[2] for x in p} == {30, 50, 100, 250} and {x[3] for x in p} == {4, 8, 150}
    for d in fuzz_inputs.DRAWS:
        (knobs, opts), (side_knobs, side_opts) = fuzz_inputs.find_knobs(d)
        assert knobs["round_phases"] in (1, 7, 256) and knobs["max_views"] in (-1, 3, 64) and knobs["predict_f"] in (1, 2, 3) and side_opts["side_lanes"] in (1, 2, 4)
        assert knobs.get("sparse_rounds", 1) in (1, -1) and opts in ({}, {"compact_pools": 2}) and side_knobs == {"max_jobs": 6}


@pytest.mark.parametrize("draw", fuzz_inputs.DRAWS)
def test_draw(pool, draw):
    d = pool.get(draw)
    _, n_seeds, n_multi, max_inst, max_count = fuzz_inputs.TABLE[draw]
    seeds, k, b, m = d.seeds, d.k, d.b, d.m
    assert len(seeds) == n_seeds
    assert int(seeds["count"].max()) == max_count
    idx = fuzz_inputs.sample(seeds, *fuzz_inputs.SAMPLE_16)
    assert set(fuzz_inputs.sample(seeds, *fuzz_inputs.SAMPLE_HUGE)[:fuzz_inputs.SAMPLE_HUGE[0]]) <= set(idx)

    # directly after find_blocks, before any set_used
    assert d.oracle_state == "final" and not d._refs["final"]
    direct = [d.orc.process_seed(k, b, m, int(seeds["vid"][i]), int(seeds["ch"][i])) for i in idx]
    chr_start = d.st.chr_start()
    assert np.array_equal(d.orc.used_bitmap(chr_start), d.states["final"])

    unused = d.refs("unused", idx)
    assert np.array_equal(d.orc.used_bitmap(chr_start), d.states["unused"]) and not d.states["unused"].any()
    sizes = [len(inst) for inst, _ in unused]
    whole = [len(inst) for inst, _ in d.refs("unused", range(n_seeds))]          # (draw 20's heaviest seed lies outside the sample)
    print("draw %d: %s, %d seeds, %d with more than one instance, most instances %d, largest count %d; %d sampled, %d of them with more than one instance"
          % (draw, (k, b, m, d.a), n_seeds, sum(s > 1 for s in whole), max(whole), int(seeds["count"].max()), len(idx), sum(s > 1 for s in sizes)))
    assert max(whole) >= max_inst and sum(s > 1 for s in whole) == n_multi
    assert sum(s > 1 for s in sizes) >= 100

    rnd = d.refs("random", idx)
    assert np.array_equal(d.orc.used_bitmap(chr_start), d.states["random"]), "set_used followed by used_bitmap returns the words written"
    n_set = int(np.unpackbits(d.states["random"].view(np.uint8)).sum())
    assert 20 <= n_set < d.st.n_positions()
    differ = sum(x != y for x, y in zip(rnd, unused))
    print("draw %d: the random state changes %d of %d sampled seeds (%d of %d positions used)" % (draw, differ, len(idx), n_set, d.st.n_positions()))
    assert differ >= 10

    assert d.refs("final", idx) == direct, "after set_used(final words) a seed gives what it gave directly after find_blocks"
    assert np.array_equal(d.orc.used_bitmap(chr_start), d.states["final"])
    assert sum(x != y for x, y in zip(direct, unused)) >= 10

    if draw == 20:          # one below the abundance limit; more instances than the compact variant's small pools hold
        assert max_count == d.a - 1 and max(whole) > 128

