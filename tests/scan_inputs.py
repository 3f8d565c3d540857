"""Two inputs that take every one-workgroup scan of the device-building routes past its first piece (tests/test_scan_inputs_cpu.py
asserts the sizes against the host route, tests/test_gpu_scan_pieces.py runs the device routes on them). Data, generated at test time
with numpy; nothing is committed.

packed(tmp): a hand-packed junction file (`<Iq` records: position, vertex id; one separator per chromosome) and its FASTA.
  * N = 2 * 2^20 + 300 * 256 + 77 raw records: 8493 blocks of 256, three pieces of graphScan with a partial last one, at both call
    sites (the file has N + 8 records).
  * Eight chromosomes at the raw indices FIRST: one starts exactly at 4096 * 256 (the first block of the second piece), the one in
    front of it - a single record - at 4096 * 256 - 1, another single record earlier, and one of 700 records that the abundance filter
    empties (two whole blocks of 256 and more). No other boundary is a multiple of 256.
  * Positions ascend in steps of 1 to 3 inside a chromosome: the FASTA has about two bases per record.
  * HOT ids take every second raw record and the emptied chromosome; `a` is below the count of each of them, so all are dropped.
  * Every kept vertex occurs exactly four times, scattered over the whole file by a multiplicative permutation of the kept index; about
    one occurrence in four has the sign set.
  * The FASTA is random ACGT with 40 lower-case n at pos + k of kept records whose kept index is beyond 2^20: the patch of the
    characters the device cannot code reaches a late index.

fasta(tmp): a FASTA for the junction finder: one record of 700 015 bases = 700 001 windows at k = 15, so that one default tile has
2735 blocks of 256 windows (three per lane of junctionScan). Eight copies of an 80 000-base random sequence with about 2 % substitutions
and a few indels each, and an unrelated random stretch of about 60 000 bases behind the fourth copy (STRETCH: its bases), whose blocks
have no junctions."""
import math
import os

import numpy as np

K = 15
N = 2 * (1 << 20) + 300 * 256 + 77
PIECE = 4096 * 256                      # raw records per piece of graphScan
FIRST = [0, 300001, 300002, 700003, 700703, PIECE - 1, PIECE, 1600001]
EMPTIED, SINGLE = 3, (1, 5)             # chromosomes
HOT = 32
N_PATCH = 40
SEP = (0xFFFFFFFF, (1 << 63) - 1)
MULT = 611953                           # the multiplier of the permutation (asserted coprime with the kept count)

WINDOWS = 700001
COPY, COPIES, AFTER = 80000, 8, 4


def _layout():
    """-> hot mask, kept raw indices, chromosome of every raw record."""
    bounds = np.array(FIRST + [N], dtype=np.int64)
    chrom = np.repeat(np.arange(len(FIRST)), np.diff(bounds))
    i = np.arange(N, dtype=np.int64)
    hot = (i % 2 == 1) | (chrom == EMPTIED)
    for c in SINGLE:
        hot[FIRST[c]] = False
    kept = np.nonzero(~hot)[0]
    if len(kept) % 4:                    # (a whole number of vertices of four occurrences: the last few kept records become hot)
        hot[kept[-(len(kept) % 4):]] = True
        kept = np.nonzero(~hot)[0]
    return hot, kept, chrom


def packed(tmp):
    """-> dict(graph, fasta=[path], k, a, raw=N, first=FIRST, kept, vertices, hot_ids, patched): the input under tmp (made once)."""
    graph, fa = os.path.join(str(tmp), "scan_packed.bin"), os.path.join(str(tmp), "scan_packed.fa")
    hot, kept, chrom = _layout()
    n_kept, n_hot = len(kept), N - len(kept)
    V = n_kept // 4
    assert n_kept == 4 * V and math.gcd(MULT, n_kept) == 1
    abundance = n_hot // HOT - 5
    assert abundance > 4
    out = dict(graph=graph, fasta=[fa], k=K, a=abundance, raw=N, first=list(FIRST), kept=n_kept, vertices=V + HOT + 1, hot_ids=(V + 1, V + HOT), patched=N_PATCH)
    if os.path.exists(graph) and os.path.exists(fa):
        return out
    rng = np.random.default_rng(20240)
    ids = np.zeros(N, dtype=np.int64)
    j = np.arange(n_kept, dtype=np.int64)
    ids[kept] = (1 + (j * MULT) % n_kept % V) * np.where(rng.integers(0, 4, n_kept) == 0, -1, 1)
    ids[hot] = V + 1 + np.arange(n_hot) % HOT
    pos = np.zeros(N, dtype=np.int64)
    step = rng.integers(1, 4, N)
    bounds = FIRST + [N]
    rec = np.dtype([("pos", "<u4"), ("id", "<i8")])
    assert rec.itemsize == 12
    parts, seqs = [], []
    for c in range(len(FIRST)):
        lo, hi = bounds[c], bounds[c + 1]
        pos[lo:hi] = np.cumsum(step[lo:hi]) - 1
        block = np.zeros(hi - lo + 1, dtype=rec)
        block["pos"][:-1], block["id"][:-1] = pos[lo:hi], ids[lo:hi]
        block["pos"][-1], block["id"][-1] = SEP
        parts.append(block)
        seqs.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(pos[hi - 1]) + K + 2)])
    # lower-case n behind the k-mer of kept records with a late kept index
    late = kept[(1 << 20) + 1:]
    assert len(late) > 10 * N_PATCH
    for r in late[:: len(late) // N_PATCH][:N_PATCH]:
        seqs[chrom[r]][pos[r] + K] = ord("n")
    tmp_graph, tmp_fa = graph + ".part", fa + ".part"
    np.concatenate(parts).tofile(tmp_graph)
    with open(tmp_fa, "wb") as f:
        for c, s in enumerate(seqs):
            f.write(b">c%d\n" % c + s.tobytes() + b"\n")
    os.replace(tmp_fa, fa)
    os.replace(tmp_graph, graph)
    return out


def _mutated(rng, base):
    s = base.copy()
    hit = rng.random(len(s)) < 0.02
    s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4              # a substitution changes the base
    for at in sorted(rng.integers(100, len(s) - 100, 6), reverse=True):
        if at % 2:
            s = np.delete(s, slice(at, at + 1 + at % 3))
        else:
            s = np.insert(s, at, rng.integers(0, 4, 1 + at % 3))
    return s


def fasta(tmp):
    """-> dict(fasta=[path], k, windows=WINDOWS, stretch=(first base, end) of the unrelated stretch): the input under tmp (made once)."""
    fa = os.path.join(str(tmp), "scan_copies.fa")
    rng = np.random.default_rng(777)
    base = rng.integers(0, 4, COPY)
    copies = [_mutated(rng, base) for _ in range(COPIES)]
    n_stretch = WINDOWS + K - 1 - sum(len(c) for c in copies)
    assert 59000 < n_stretch < 61100
    stretch = rng.integers(0, 4, n_stretch)
    seq = np.concatenate(copies[:AFTER] + [stretch] + copies[AFTER:])
    assert len(seq) == WINDOWS + K - 1
    lo = sum(len(c) for c in copies[:AFTER])
    if not os.path.exists(fa):
        with open(fa + ".part", "wb") as f:
            f.write(b">copies\n" + np.frombuffer(b"ACGT", dtype=np.uint8)[seq].tobytes() + b"\n")
        os.replace(fa + ".part", fa)
    return dict(fasta=[fa], k=K, windows=WINDOWS, stretch=(lo, lo + n_stretch))
