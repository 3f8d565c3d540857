"""The resolved heavy vote of the wide and big variants (lcb_vote_resolve / lcb_vote_items, csrc/lcb_kernel.h) on the device: votes of
LCB_VOTE_RESOLVE_MIN .. LCB_VOTE_RESOLVE_MAX voters in the 16-wavefront variants are resolved by wave 0 and dealt as (voter, chunk)
items. The input is the synthetic one of tests/test_vote_resolve_emu.py - 70 strains, so that a vote has more than 64 voters and windows
of several 64-step chunks; which path a vote takes depends only on its number of voters, so the emulator's event counters vouch that
the resolved path runs on it. Checked against the CPU oracle: per-seed results in both `used` states, and the whole FindBlocks."""
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from tests.oracle_binding import Oracle

pytestmark = pytest.mark.gpu

K, B, M, A = 15, 200, 50, 150
# bench.py's config-3 generator parameters at 70 strains and 4 segments (tests/test_vote_resolve_emu.py names the same input)
SYNTH = ("--strains 70 --segments 4 --keep 0.8 --swap 0.05 --invert 0.10 --sub 0.02 --indel 0.002 --filler-frac 0.25 --filler-min 200 --filler-max 3000 "
         "--repeat-families 3 --repeat-copies 10 --repeat-len 800 --seg-min 500 --seg-max 8000 --seed 9101")
N_SEEDS = 400          # the heavy head of the seed order: the seeds of the most occurrences, i.e. of the most voters


@pytest.fixture(scope="module")
def synth(built, tmp_path_factory):
    """The input, its storage and the oracle's answers (computed once, shared by the tests, never changed)."""
    import bench
    d = tmp_path_factory.mktemp("vote_resolve")
    fa, gr = str(d / "g.fa"), str(d / "g.bin")
    subprocess.check_call([os.path.join(bench.BIN, "lcb-synth"), "-o", fa] + SYNTH.split())
    subprocess.check_call([os.path.join(bench.BIN, "lcb-mkgraph"), "-k", str(K), "-o", gr, fa], stderr=subprocess.DEVNULL)
    st = sibeliaz_amd.JunctionStorage(gr, [fa], K, threads=4, abundance=A)
    seeds = st.seeds(4)
    assert os.path.getsize(fa) < 4 << 20 and len(seeds) > N_SEEDS
    head = seeds[:N_SEEDS]
    orc = Oracle(gr, [fa], K, A)
    ref = {"unused": [orc.process_seed(K, B, M, int(s["vid"]), int(s["ch"])) for s in head]}
    blocks, stats = orc.find_blocks(K, B, M)
    final = np.array(orc.used_bitmap(st.chr_start()), dtype="<u4")
    ref["final"] = [orc.process_seed(K, B, M, int(s["vid"]), int(s["ch"])) for s in head]
    return dict(st=st, seeds=seeds, head=head, ref=ref, final=final, blocks=blocks, stats=stats)


@pytest.mark.parametrize("state", ["unused", "final"])
@pytest.mark.parametrize("mode", [2, 3])
def test_per_seed_parity(synth, mode, state):
    """Every seed of the heavy head through the wide (2) / big (3) variant against the oracle."""
    p = sibeliaz_amd.Params.make(K, b=B, m=M)
    dev = sibeliaz_amd.Device(synth["st"], p, 0, start_mode=mode)
    try:
        if state == "final":
            dev.set_used(synth["final"])
        off, inst, score, _ = dev.process_seeds(synth["head"])
        counts = dev.mode_seeds()
    finally:
        dev.close()
    bad = []
    for i, (ref, ref_score) in enumerate(synth["ref"][state]):
        got = inst[int(off[i]):int(off[i + 1])]
        tup = [(int(a["chr"]), int(a["front_idx"]), int(a["back_idx"]), int(a["positive"]) != 0) for a in got]
        if tup != ref or int(score[i]) != ref_score:
            bad.append(i)
    assert not bad, "%d of %d seeds differ from the oracle (variant %d, %s state), first %s" % (len(bad), N_SEEDS, mode, state, bad[:5])
    assert counts[mode - 1] >= N_SEEDS and all(c == 0 for c in counts[:mode - 1]), counts


@pytest.mark.parametrize("mode", [2, 3])
def test_find_blocks_matches_the_oracle(synth, mode):
    """The whole FindBlocks with every seed in the wide / big variant against the oracle's."""
    p = sibeliaz_amd.Params.make(K, b=B, m=M)
    dev = sibeliaz_amd.Device(synth["st"], p, 0, start_mode=mode)
    try:
        finder = sibeliaz_amd.BlocksFinder(synth["st"], K)
        blocks = finder.FindBlocks(M, B, device=dev, seeds=synth["seeds"], threads=4)
        stats = dict(finder.stats)
    finally:
        dev.close()
    ref = synth["blocks"]
    assert len(blocks) == len(ref)
    for f in ("id", "chr", "start", "end"):
        assert np.array_equal(np.asarray(blocks[f], dtype=np.int64), np.asarray(ref[f], dtype=np.int64)), f
    assert stats["blocks_found"] == synth["stats"]["blocks_found"] and stats["failures"] == synth["stats"]["failures"]
