"""Synthetic inputs that reach the pool limits of the kernel variants by themselves (CPU emulator and GPU): the capacity ladder compact -> wide ->
big -> huge -> doubled huge, which no golden and no other synthetic input of the suite climbs without a forced variant or a shrunk path set.
Data, generated at test time, in the style of tests/seed_inputs.py (k = 15, graph by the CPU lcb-mkgraph); b = 200, m = 50.

The pools (lcb_kernel.h, LcbCfg): instances 128 (compact, small pools) / 256 (compact) / 1 024 (wide) / 4 096 (big) / 8 192 (huge, doubling);
vote tables 512 / 1 024 / 2 048 / 4 096 / 65 536 slots, of which three quarters may be claimed. (The result snapshot holds as many entries as the
instance pool in every variant, so it never fills before the pool does: no input here aims at it.)

joiners(n1, n2, n_records, rc_every, seed): R1 and R2 are 60 random bases each; n1 parts R1+R2 and n2 parts R2 alone, shuffled; part i is
reverse-complemented when i % rc_every == rc_every - 1, follows 40 fresh random bases and goes to record i % n_records; every record ends with 40
random bases. A seed at a junction of R2 starts with n1 + n2 instances (the pool fills when the path is initialised), one at a junction of R1 starts
with n1 and gains n2 when the path reaches R2 (the pool fills in a push): the two places where the instance pool overflows.

tails(n, motifs_per, motif_len, n_records, seed): R is 60 random bases; a library of n * motifs_per / 2 random motifs, every motif used exactly
twice, in the tails of two different copies (the slots are shuffled); copy i is 40 random bases, R, then motifs_per x (motif + 3 random bases), in
record i % n_records; no reverse complements. The look-ahead windows behind R hold many distinct junction vertices per voter while the pool holds
few instances: the vote table fills first."""
import random

from tests.seed_inputs import ABUNDANCE, K, _rc, _seq, write_input

B, M = 200, 50
VARIANTS = ("compact", "wide", "big", "huge")

HUGE_IC = 8192   # instances of a huge slot before its first doubling
HEAVY = 8      # the "heaviest seeds" of a tails input: the first 8 of the seed order (where a vote-table exit is asserted to be a PURE one, it is for these)

# (n1, n2, n_records, rc_every) -> the variants its heaviest seeds leave with a full instance pool, by the pools of the compact variant (1 = 256
# instances, 2 = 128), and the doublings of the huge workspace (8 192 instances at first) they need. The pool of such a seed reaches
# about twice its occurrence count (the path passes R1 and R2 of both strands), so (120, 10) leaves the 256-instance pool too and (4090, 10) needs
# 16 384 instances.
# The emulator is deterministic and doubles exactly that often; the device may not do it less often. Measured with the emulator; every test asserts it again before it relies on it.
JOINERS = {
    (120, 10, 5, 3): {1: ("compact",), 2: ("compact",), "grow": 0},
    (250, 10, 5, 3): {1: ("compact",), 2: ("compact",), "grow": 0},
    (1000, 30, 5, 3): {1: ("compact", "wide"), 2: ("compact", "wide"), "grow": 0},
    (4090, 10, 5, 3): {1: ("compact", "wide", "big", "huge"), 2: ("compact", "wide", "big", "huge"), "grow": 1},
    (8190, 5, 5, 3): {1: ("compact", "wide", "big", "huge"), 2: ("compact", "wide", "big", "huge"), "grow": 2},
    (8200, 5, 5, 3): {1: ("compact", "wide", "big", "huge"), 2: ("compact", "wide", "big", "huge"), "grow": 2},
}
# the last one is for the device's growth path alone: its heaviest seeds yield 8 200 instances, more than the snapshot buffer of the huge workspace holds
# before it has doubled too (8 192) - the blocks of (8190, 5) have 8 190 and would fit a snapshot buffer that the doubling forgot
SNAPSHOT_EDGE = (8200, 5, 5, 3)
JOINERS_LARGE = (16380, 10, 5, 3)          # (by hand, on the emulator only: three doublings)

# (n, motifs_per, motif_len, n_records) -> by the pools of the compact variant, the variants that seeds of the heavy head leave with a full VOTE TABLE,
# and ("pure") those that none of the HEAVY heaviest leaves with a full instance pool: the vote-table exit with the pool within its limits
TAILS = {
    (100, 8, 20, 5): {1: ("compact",), 2: ("compact",), "pure": ("compact",)},
    (60, 8, 20, 5): {1: (), 2: ("compact",), "pure": ("compact",)},
    (500, 4, 20, 5): {1: ("compact", "wide"), 2: ("compact", "wide"), "pure": ("wide",)},
    (1500, 4, 20, 5): {1: ("wide", "big"), 2: ("wide", "big"), "pure": ("big",)},
}

# The claim limit itself: tails(46, 8, 20, 5, seed=2) has a seed one of whose votes meets exactly 385 distinct candidates, one more than three quarters of the
# 512 slots of the small compact pools. Of the first 150 seeds 26 leave the compact variant because of the vote table (none because of the pool); with a
# limit one larger it is 25. (params, seed, seeds, exits): measured with the emulator, the same on the device.
CLAIM_EDGE = ((46, 8, 20, 5), 2, 150, 26)


def joiners_text(n1, n2, n_records, rc_every, seed=1):
    rng = random.Random(seed * 1000003 + n1 * 31 + n2)
    r1, r2 = _seq(rng, 60), _seq(rng, 60)
    kinds = [r1 + r2] * n1 + [r2] * n2
    rng.shuffle(kinds)
    rec = [[] for _ in range(n_records)]
    for i, body in enumerate(kinds):
        rec[i % n_records].append(_seq(rng, 40) + (_rc(body) if i % rc_every == rc_every - 1 else body))
    return "".join(">r%d\n%s%s\n" % (j, "".join(parts), _seq(rng, 40)) for j, parts in enumerate(rec))


def tails_text(n, motifs_per, motif_len, n_records, seed=1):
    rng = random.Random(seed * 1000003 + n * 31 + motifs_per)
    r = _seq(rng, 60)
    n_motifs = n * motifs_per // 2
    motifs = [_seq(rng, motif_len) for _ in range(n_motifs)]
    # every motif twice, in two DIFFERENT copies: shuffle, then repair the few copies that drew a motif twice by swapping with a neighbour
    slots = list(range(n_motifs)) * 2
    rng.shuffle(slots)
    for _ in range(8):
        clash = False
        for c in range(n):
            own = slots[c * motifs_per:(c + 1) * motifs_per]
            for j, mo in enumerate(own):
                if own.index(mo) != j:
                    a, b = c * motifs_per + j, ((c + 1) % n) * motifs_per + j
                    slots[a], slots[b] = slots[b], slots[a]
                    clash = True
        if not clash:
            break
    rec = [[] for _ in range(n_records)]
    for i in range(n):
        tail = "".join(motifs[mo] + _seq(rng, 3) for mo in slots[i * motifs_per:(i + 1) * motifs_per])
        rec[i % n_records].append(_seq(rng, 40) + r + tail)
    return "".join(">r%d\n%s%s\n" % (j, "".join(parts), _seq(rng, 40)) for j, parts in enumerate(rec))


def joiners(tmp, n1, n2, n_records, rc_every, seed=1):
    return write_input(tmp, "joiners_%d_%d_%d_%d_%d" % (n1, n2, n_records, rc_every, seed), joiners_text(n1, n2, n_records, rc_every, seed))


def tails(tmp, n, motifs_per, motif_len, n_records, seed=1):
    return write_input(tmp, "tails_%d_%d_%d_%d_%d" % (n, motifs_per, motif_len, n_records, seed), tails_text(n, motifs_per, motif_len, n_records, seed))


def parse_ladder(stderr):
    """The emulator's `ladder:` lines -> ({variant: {"ok", "inst", "vote", "path", "best", "clash", "nw"}}, [huge capacities after each doubling]); clash: the
    instance-pool exits with the pool not full (a footprint slot across two segments), nw: the set of wavefront counts the variant was launched with."""
    exits = {v: dict(ok=0, inst=0, vote=0, path=0, best=0, clash=0, nw=set()) for v in VARIANTS}
    grown = []
    for ln in stderr.splitlines():
        f = ln.split()
        if f[:2] == ["ladder:", "mode"]:
            e = exits[VARIANTS[int(f[2])]]
            for key, val in zip(f[3::2], f[4::2]):
                if key == "nw":                                  # the wavefronts of the launch: every one a variant was run with
                    e["nw"].add(int(val))
                elif key != "cap":                               # (`cap`: the instance pool of the launch)
                    e[key] += int(val)
        elif f[:4] == ["ladder:", "huge", "grown", "to"]:
            grown.append(int(f[4]))
    return exits, grown


def check_property(kind, params, seeds, exits=None, grown=None, pools=1, segmented=False, heavy_only=False, start="compact"):
    """What a test relies on when it uses joiners(*params) / tails(*params): asserted against the HOST enumerator's seeds (a structured array) and,
    where the caller has them, against the exits the run reported per variant - the emulator's `ladder:` lines through parse_ladder, or
    Device.overflows()["counts"] through device_exits - and the huge capacities after each doubling. heavy_only: the run held no more than the HEAVY
    heaviest seeds (and any number of light ones), so the pure vote-table exits are asserted too. start: the variant the seeds began in."""
    top = int(seeds["count"].max())
    if exits is not None and not segmented:      # without segments a pool is full when a seed leaves because of it
        assert all(e.get("clash", 0) == 0 for e in exits.values()), "%s%r: a seed left a variant with the pool status and the pool not full: %r" % (kind, params, exits)
    if exits is not None:        # the snapshot buffer holds as many entries as the instance pool in every variant (and doubles with it): it never fills first
        assert all(e["best"] == 0 for e in exits.values()), "%s%r: a seed left a variant with a full result snapshot: %r" % (kind, params, exits)
    if kind == "joiners":
        assert top == params[0] + params[1], "joiners%r: the largest count is %d" % (params, top)
        if exits is None:
            return
        left = JOINERS[params][pools]
        for v in VARIANTS[VARIANTS.index(start):]:
            if v in left:
                assert exits[v]["inst"] > 0, "joiners%r: no seed left %s with a full instance pool: %r" % (params, v, exits)
            elif not segmented:      # (with segments a footprint slot shared across segments also ends a seed with this status)
                assert exits[v]["inst"] == 0 and exits[v]["vote"] == 0, "joiners%r: a seed left %s: %r" % (params, v, exits)
        if grown is not None:
            assert len(grown) == JOINERS[params]["grow"], "joiners%r: the huge workspace doubled %d times, %d expected" % (params, len(grown), JOINERS[params]["grow"])
    else:
        assert top == params[0], "tails%r: the largest count is %d" % (params, top)
        if exits is None:
            return
        for v in VARIANTS:
            if v in TAILS[params][pools]:
                assert exits[v]["vote"] > 0, "tails%r: no seed left %s with a full vote table: %r" % (params, v, exits)
                if heavy_only and v in TAILS[params]["pure"]:
                    assert exits[v]["inst"] == 0, "tails%r: a seed left %s with a full instance pool: %r" % (params, v, exits)
        if not TAILS[params][pools]:
            assert all(exits[v]["vote"] == 0 and exits[v]["inst"] == 0 for v in VARIANTS), "tails%r: a seed left a variant: %r" % (params, exits)
        assert exits["huge"]["vote"] == 0 and exits["huge"]["inst"] == 0, "tails%r: a seed left the huge variant: %r" % (params, exits)


def device_exits(overflows):
    """Device.overflows() in the shape of parse_ladder's first result."""
    return {v: dict(inst=c["instances"], vote=c["vote"], path=c["path"], best=c["snapshot"]) for v, c in overflows["counts"].items()}


assert ABUNDANCE and K      # (re-exported for the tests: one place names the graph parameters)
