"""Synthetic inputs for the seed-enumeration tests (CPU emulator and GPU): vertices with long occurrence lists, which no golden has (the
largest count of a golden seed is 17, so none of their lists spans two 64-occurrence chunks of the device code). Data, generated at test time.

heavy(n_copies, n_records, rc_every, n_every, seed): R = 60 random bases; copy i goes to record i % n_records behind 40 fresh random
bases, reverse-complemented when i % rc_every == rc_every - 1, followed by a lower-case `n` when n_every != 0 and i % n_every == 0; every
record ends with 40 random bases. k = 15, graph by the CPU lcb-mkgraph. The junctions inside R then occur n_copies times each."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MKGRAPH = os.path.join(ROOT, "sibeliaz_amd", "bin", "lcb-mkgraph")
K = 15
ABUNDANCE = 1000000

# (n_copies, n_records, rc_every, n_every): the property each stands for is asserted by the tests that use it, against the host enumerator
HEAVY = [(63, 3, 4, 0), (64, 3, 4, 0), (65, 3, 4, 0), (257, 5, 3, 0), (1000, 7, 2, 0), (300, 300, 5, 0), (400, 5, 3, 2)]
FILTERED = ((400, 5, 3, 2), 150)          # the same input at abundance 150: the filtered CSR


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def heavy_text(n_copies, n_records, rc_every, n_every, seed=1):
    rng = random.Random(seed * 1000003 + n_copies * 31 + n_records)
    r = _seq(rng, 60)
    rec = [[] for _ in range(n_records)]
    for i in range(n_copies):
        part = _seq(rng, 40) + (_rc(r) if i % rc_every == rc_every - 1 else r)
        if n_every and i % n_every == 0:
            part += "n"
        rec[i % n_records].append(part)
    return "".join(">r%d\n%s%s\n" % (j, "".join(parts), _seq(rng, 40)) for j, parts in enumerate(rec))


def write_input(tmp, name, text, k=K):
    """FASTA + graph of `text` under tmp; returns (graph, fasta)."""
    fasta = os.path.join(str(tmp), name + ".fa")
    graph = os.path.join(str(tmp), name + ".bin")
    if not os.path.exists(graph):
        with open(fasta, "w") as f:
            f.write(text)
        subprocess.check_call([MKGRAPH, "-k", str(k), "-o", graph, fasta], stderr=subprocess.DEVNULL)
    return graph, fasta


def heavy(tmp, n_copies, n_records, rc_every, n_every, seed=1):
    name = "heavy_%d_%d_%d_%d_%d" % (n_copies, n_records, rc_every, n_every, seed)
    return write_input(tmp, name, heavy_text(n_copies, n_records, rc_every, n_every, seed))


def no_seed(tmp):
    """One random record: no vertex occurs twice."""
    return write_input(tmp, "no_seed", ">only\n%s\n" % _seq(random.Random(5), 3000))


def check_property(params, abundance, seeds):
    """What a test relies on when it uses heavy(*params): asserted against the HOST enumerator's seeds (a structured array)."""
    n_copies, n_records, rc_every, n_every = params
    if abundance == ABUNDANCE:
        assert int(seeds["count"].max()) >= n_copies, "heavy%r: the largest count is %d" % (params, int(seeds["count"].max()))
    else:
        assert 64 < int(seeds["count"].max()) < n_copies, "heavy%r at abundance %d: the filter does not bite" % (params, abundance)
    if n_records >= 257:
        assert int(seeds["resolve_chr"].max()) >= 256, "heavy%r: resolve_chr fits one byte" % (params,)
    if n_every and abundance == ABUNDANCE:      # (the vertices in front of an `n` occur too often for the filter)
        acgt = [ord(c) for c in "ACGTacgt"]
        assert any(int(c) not in acgt for c in seeds["ch"]), "heavy%r: every character is ACGT" % (params,)
        assert (seeds["vid"] < 0).any(), "heavy%r: no seed with a negative vertex id" % (params,)
