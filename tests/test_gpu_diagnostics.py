"""The diagnostic flavour of the launch path (run with -m gpu on an MI355X): the instrumented (`prof`) kernel instantiations, the
bounded wait of a launch and the launch trace, which nothing else in the suite runs. On the first 300 seeds of every golden case and
for every kernel variant as the starting one, a Device created under LCB_FORCE_PROF=1, LCB_TRACE_SEEDS=1, LCB_DEBUG=1,
LCB_TRACE_LAUNCHES=<file> and LCB_WATCHDOG_S=120 (far above any launch here: it only makes the wait poll) returns what a default
Device returns, writes one well-formed trace line per launch, and refuses the overlapped launch of process_begin."""
import numpy as np
import pytest

import sibeliaz_amd

pytestmark = pytest.mark.gpu

N_SEEDS = 300
VARIANTS = ("compact", "wide", "big", "huge")
SEED_KEYS = "st= n= ticks= push= vote= probe= inst= tv= tp= ts= cwalk= cwaitb= creduce= cscan= voters= chunks= touch=".split()
_default = {}       # case name -> what a default Device returns for the case's first seeds (computed once, never changed)


def _storage(case):
    st = sibeliaz_amd.JunctionStorage(case.graph, [case.fasta], case.k, threads=4, abundance=case.a)
    return st, sibeliaz_amd.Params.make(case.k, b=case.b, m=case.m)


def _default_results(case):
    if case.name not in _default:
        st, p = _storage(case)
        seeds = st.seeds(4)[:N_SEEDS]
        dev = sibeliaz_amd.Device(st, p, 0)
        off, inst, score, _ = dev.process_seeds(seeds)
        dev.close()
        _default[case.name] = (seeds, off, inst, score)
    return _default[case.name]


def _instrument(monkeypatch, trace):
    for k, v in (("LCB_FORCE_PROF", "1"), ("LCB_TRACE_SEEDS", "1"), ("LCB_DEBUG", "1"), ("LCB_TRACE_LAUNCHES", str(trace)), ("LCB_WATCHDOG_S", "120")):
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_instrumented_launches_equal_the_default_and_are_traced(built, case, mode, tmp_path, monkeypatch):
    seeds, off0, inst0, score0 = _default_results(case)
    trace = tmp_path / "launches.tsv"
    _instrument(monkeypatch, trace)
    st, p = _storage(case)
    dev = sibeliaz_amd.Device(st, p, 0, start_mode=mode)
    off, inst, score, _ = dev.process_seeds(seeds)
    _, launches = dev.kernel_time()
    dev.close()
    assert np.array_equal(off, off0) and np.array_equal(inst, inst0) and np.array_equal(score, score0)
    lines = trace.read_text().splitlines()
    rows = [ln.split("\t") for ln in lines if not ln.startswith("#")]
    print("%s start_mode %d: %d launches, %d #seed lines" % (case.name, mode, launches, len(lines) - len(rows)))
    assert launches >= 1 and len(rows) == launches
    for i, r in enumerate(rows):
        assert len(r) == 5, r
        assert int(r[0]) == i + 1, r                                  # a running launch number from 1
        assert 1 <= int(r[2]) <= int(r[1]) <= len(seeds), r           # seeds, grid <= seeds
        assert r[3] in VARIANTS, r
        assert float(r[4]) >= 0.0, r
    assert int(rows[0][1]) == len(seeds) and rows[0][3] == VARIANTS[mode - 1], rows[0]     # the first launch: every seed in the chosen variant
    profiled = set()      # launches with a per-seed profile line: only the prof instantiations write the counters behind it
    for ln in lines:
        if ln.startswith("#seed"):
            f = ln.split("\t")
            assert f[0] == "#seed" and 1 <= int(f[1]) <= launches and 0 <= int(f[2]) < len(seeds), ln
            int(f[3])
            assert [x[: x.index("=") + 1] for x in f[4:]] == SEED_KEYS, ln
            assert all(int(x[x.index("=") + 1:]) >= 0 for x in f[4:]), ln
            assert int(f[6][len("ticks="):]) > 2000, ln                   # the writer's threshold: 20 us of a seed's own clock
            profiled.add(int(f[1]))
        else:
            assert not ln.startswith("#"), ln
    # the prof flavour really ran: every launch has a seed that took more than 20 us by the in-kernel timers (with the flight
    # recorder on every seed of these cases does); the plain flavour would leave the counters zero and write no such line
    assert profiled == set(range(1, launches + 1)), (sorted(profiled), launches)


def test_process_begin_refuses_while_instrumented(built, case, tmp_path, monkeypatch):
    """The instrumented variants share one profile buffer, so the overlapped launch is not taken: a FindBlocks on such a device
    reports no early critical launch (and finds the blocks of a default device)."""
    st, p = _storage(case)
    finder = sibeliaz_amd.BlocksFinder(st, case.k)
    dev0 = sibeliaz_amd.Device(st, p, 0)
    blocks0 = finder.FindBlocks(case.m, case.b, device=dev0, threads=2).copy()
    dev0.close()
    _instrument(monkeypatch, tmp_path / "launches.tsv")
    dev = sibeliaz_amd.Device(st, p, 0)
    blocks = finder.FindBlocks(case.m, case.b, device=dev, threads=2).copy()
    stats = dict(finder.stats)
    dev.close()
    assert stats["early_critical"] == 0, stats
    assert np.array_equal(blocks, blocks0)
