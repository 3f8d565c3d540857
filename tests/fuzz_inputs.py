"""Data helpers of the randomized parity campaign's full-size draws (tests/emu/fuzz.py, case_params(i, small=False)) - no tests here.
tests/test_fuzz_inputs_cpu.py checks with the oracle alone that the draws are what the table below says and that the sampled seeds and
the `used` states have something to compare; tests/test_gpu_fuzz.py runs them on the device against the oracle. Every input is generated
at test time with lcb-synth and the CPU lcb-mkgraph; nothing of it is committed."""
import importlib.util
import os
import subprocess

import numpy as np

from tests.oracle_binding import Oracle, OrcCounters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("lcb_fuzz", os.path.join(ROOT, "tests", "emu", "fuzz.py"))
fuzz = importlib.util.module_from_spec(spec)
spec.loader.exec_module(fuzz)

DRAWS = [2, 7, 9, 11, 13, 20, 29, 34, 37, 43, 50, 53, 55, 56]
# draw: ((k, b, m, a), seeds, seeds of the whole order with more than one instance in the unused state, most instances of a seed,
# largest count of a seed) - measured with the oracle. The generator and case_params are deterministic: the seed count is exact, and a
# change of either has to be noticed (tests/test_fuzz_inputs_cpu.py) and this table updated on purpose.
TABLE = {
    2: ((11, 200, 50, 150), 1580, 1560, 20, 16),
    7: ((25, 40, 30, 150), 1094, 1071, 25, 24),
    9: ((21, 100, 50, 150), 3969, 3953, 42, 40),
    11: ((25, 100, 50, 150), 2551, 2517, 28, 28),
    13: ((15, 100, 50, 4), 1506, 1350, 4, 3),
    20: ((21, 40, 100, 150), 1852, 686, 131, 149),
    29: ((21, 200, 30, 150), 1343, 1342, 23, 23),
    34: ((11, 100, 30, 8), 864, 688, 9, 7),
    37: ((11, 200, 250, 150), 4508, 3800, 21, 30),
    43: ((15, 400, 100, 150), 1994, 1892, 11, 9),
    50: ((21, 100, 250, 8), 1481, 421, 7, 7),
    53: ((25, 400, 100, 150), 2445, 2129, 11, 8),
    55: ((15, 200, 30, 150), 1339, 1304, 19, 15),
    56: ((25, 200, 250, 150), 743, 568, 12, 17),
}
STATES = ("unused", "random", "final")
# positions per run of used positions in the `random` state (one run of 20 to 300 positions per so many positions); a draw whose sampled
# seeds would not notice the default gets denser runs here (tests/test_fuzz_inputs_cpu.py asks for 10 sampled seeds that differ)
RANDOM_RUN_EVERY = 2000
RANDOM_RUN_EVERY_OF = {}
SAMPLE_16 = (300, 100)        # head, rest of the 16-wavefront variants (wide, big)
SAMPLE_HUGE = (150, 50)       # ... of the huge variant: one seed per CU or fewer makes every launch slow
COMPACT_POOLS_SMALL = 2       # lcb_device_opts.compact_pools: 128 instances / 512 vote slots


def generate(draw, directory):
    """-> (fasta, graph) of the draw, written once into `directory`."""
    synth, (k, b, m, a), _, _ = fuzz.case_params(draw, small=False)
    fa, gr = os.path.join(str(directory), "d%d.fa" % draw), os.path.join(str(directory), "d%d.bin" % draw)
    if not os.path.exists(gr):
        subprocess.check_call([os.path.join(fuzz.BIN, "lcb-synth"), "-o", fa] + synth, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        subprocess.check_call([os.path.join(fuzz.BIN, "lcb-mkgraph"), "-k", str(k), "-o", gr, fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return fa, gr


def sample(seeds, head, rest):
    """Indices into the sorted seed order: the first `head` seeds (the most occurrences, the most voters), then every
    ceil((n - head) / rest)-th of the remainder, so that the light seeds are not left out."""
    n = len(seeds)
    idx = list(range(min(head, n)))
    if n > head:
        idx += list(range(head, n, -(-(n - head) // rest)))
    return np.asarray(idx, dtype=np.int64)


def used_states(st, orc, k, b, m, rng, run_every=RANDOM_RUN_EVERY):
    """-> {"unused", "random", "final"}: `used` bitmaps as <u4 words in the layout Device.set_used takes (and Oracle.used_bitmap gives).
    random: runs of 20 to 300 used positions, one per `run_every` positions; final: after orc.find_blocks, which leaves the oracle there."""
    n_pos = st.n_positions()
    words = n_pos // 32 + 2
    bits = np.zeros(words * 32, dtype=bool)
    for _ in range(max(1, n_pos // run_every)):
        q = int(rng.integers(0, n_pos))
        bits[q:q + int(rng.integers(20, 300))] = True
    bits[n_pos:] = False
    orc.reset_used()
    orc.find_blocks(k, b, m)
    final = np.array(orc.used_bitmap(st.chr_start()), dtype="<u4")
    assert len(final) == words
    return {"unused": np.zeros(words, dtype="<u4"), "random": np.packbits(bits, bitorder="little").view("<u4").copy(), "final": final}


def find_knobs(draw):
    """The engine knobs and device options of the draw's first `find` run and of its side-lane run under the product's names:
    -> ((knobs, device_opts), (knobs, device_opts))."""
    runs = fuzz.case_params(draw, small=False)[2]
    finds = [env for mode, env in runs if mode == "find"]
    first, side = finds[0], next(env for env in finds if "EMU_SIDE_LANES" in env and "EMU_SEG_CAP" not in env)
    knobs = {"round_fixed": 1, "round_phases": int(first["EMU_ROUNDS"]), "max_views": int(first["EMU_VIEWS"]) or -1, "predict_f": int(first["LCB_PREDICT_F"])}
    if "LCB_SPARSE_ROUNDS" in first:
        knobs["sparse_rounds"] = int(first["LCB_SPARSE_ROUNDS"])
    opts = {"compact_pools": COMPACT_POOLS_SMALL} if "EMU_COMPACT_SMALL" in first else {}
    return (knobs, opts), ({"max_jobs": 6}, {"side_lanes": int(side["EMU_SIDE_LANES"])})


class Draw:
    """One draw: files, storage, seeds, the three `used` states and the oracle's answers per (state, seed index) - computed when first
    asked for, kept, never changed. Has the attributes of conftest.Case that the shared helpers read (name, graph, fasta, k, b, m, a)."""

    def __init__(self, draw, directory):
        import sibeliaz_amd
        self.draw, self.name = draw, "draw%d" % draw
        (self.k, self.b, self.m, self.a) = fuzz.case_params(draw, small=False)[1]
        self.fasta, self.graph = generate(draw, directory)
        self.st = sibeliaz_amd.JunctionStorage(self.graph, [self.fasta], self.k, threads=4, abundance=self.a)
        self.seeds = self.st.seeds(4)
        self.orc = Oracle(self.graph, [self.fasta], self.k, self.a)
        self.states = used_states(self.st, self.orc, self.k, self.b, self.m, np.random.default_rng(draw), RANDOM_RUN_EVERY_OF.get(draw, RANDOM_RUN_EVERY))
        self.oracle_state = "final"          # as find_blocks left it, not yet through Oracle.set_used
        self._refs = {s: {} for s in STATES}
        self._blocks = None

    def oracle_in(self, state):
        if self.oracle_state != state:
            self.orc.set_used(self.states[state], self.st.chr_start())
            self.oracle_state = state

    def refs(self, state, idx):
        """[(instances, score)] of seeds[idx] in `state`; the oracle runs once per (state, index)."""
        have = self._refs[state]
        for i in idx:
            i = int(i)
            if i not in have:
                self.oracle_in(state)
                oc = OrcCounters()
                inst, score = self.orc.process_seed(self.k, self.b, self.m, int(self.seeds["vid"][i]), int(self.seeds["ch"][i]), counters=oc)
                have[i] = (inst, score, oc.as_dict())
        return [have[int(i)][:2] for i in idx]

    def counters(self):
        """The sum of the oracle's event counters over every seed in the unused state."""
        self.refs("unused", range(len(self.seeds)))
        total = OrcCounters().as_dict()
        for _, _, c in self._refs["unused"].values():
            for name in total:
                total[name] += c[name]
        return total

    def blocks(self):
        """(blocks, stats) of the oracle's whole FindBlocks from the unused state."""
        if self._blocks is None:
            self.orc.reset_used()
            self._blocks = self.orc.find_blocks(self.k, self.b, self.m)
            self.oracle_state = "final"
        return self._blocks


class DrawPool:
    """The draws of one test session, each made when first asked for, in one directory."""

    def __init__(self, directory):
        self.directory, self._draws = str(directory), {}

    def get(self, draw):
        if draw not in self._draws:
            self._draws[draw] = Draw(draw, self.directory)
        return self._draws[draw]
