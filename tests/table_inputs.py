"""Synthetic inputs for the table-build tests (CPU emulator and GPU): junction files written directly - a junction file is only `<Iq`
records (position, vertex id) plus a separator record per sequence - next to a random FASTA long enough for them. Data, generated at
test time; the host loader (csrc/graph.cpp) accepts such files, a chromosome whose records the abundance filter removes entirely included.

An input is (pattern, P): P positions survive the filter, laid out as chromosomes of 1 position next to ones of about a sort tile, with one
chromosome in between whose `abundance` records of a vertex of its own are all dropped (chrStart[c + 1] == chrStart[c]). The gaps between
consecutive positions of a chromosome mix dense runs (step 1: the look-ahead window is limited by max_branch steps), short steps, and
sparse stretches (step 1000: window 0), starting at another phase in every chromosome so that both meet chromosome starts and ends."""
import os
import random

import numpy as np

TILE = 1024          # T_TILE of lcb_table_kernels.h: the records of one workgroup of the scatter kernel
K = 15
SIZES = [TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
PATTERNS = ["one_vertex", "distinct", "both_signs", "high_byte", "long_list"]
MAX_BRANCH = [12, 400]
MAX_ID = 1 << 20
SEP = (0xFFFFFFFF, (1 << 63) - 1)
_PHASE = [0, 40, 41, 58, 20]


def ids(pattern, n):
    """Vertex ids (1 <= |id| < 2^20) of the n kept positions, in flat order."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "one_vertex":          # one list with everything
        return np.full(n, 7, dtype=np.int64)
    if pattern == "distinct":            # every list has one entry
        return i + 1
    if pattern == "both_signs":
        return ((i * 7) % 97 + 1) * np.where(i % 3 == 0, -1, 1)
    if pattern == "high_byte":           # the ids differ in byte 2 only: three of the four digits are skipped
        return 5 + (((i * 5) % 15) << 16)
    if pattern == "long_list":           # three quarters of the positions in one list (longer than a tile at the largest size), the rest in short ones
        return np.where(i % 4 != 0, 3, (10 + i % 50) * np.where(i % 8 == 0, -1, 1))
    raise KeyError(pattern)


def chromosome_sizes(n):
    """Kept positions per chromosome; None marks the chromosome that the filter empties."""
    a = min(1000, n - 3)
    rest = n - 2 - a
    tail = [rest] if rest <= 1500 else [rest - 1100, 1100]
    return [1, a, None, 1] + tail


def _positions(n, c):
    phase = (np.arange(n - 1) + _PHASE[c % len(_PHASE)]) % 64
    step = np.where(phase < 40, 1, np.where(phase < 44, 1000, np.where(phase < 60, 5, 13)))
    return np.concatenate([[c % 3], (c % 3) + np.cumsum(step)]).astype(np.int64)[:n]


def write(tmp, pattern, n):
    """-> dict(graph, fasta, k, a, positions, vertices, empty_chr): the input (pattern, n) under tmp."""
    name = "%s_%d" % (pattern, n)
    graph, fasta = os.path.join(str(tmp), name + ".bin"), os.path.join(str(tmp), name + ".fa")
    vid = ids(pattern, n)
    assert vid.min() >= -MAX_ID and vid.max() <= MAX_ID and (vid != 0).all()
    abundance = n + 1                    # more than any kept vertex can have
    empty_id = int(np.abs(vid).max()) + 1
    assert empty_id <= MAX_ID
    sizes = chromosome_sizes(n)
    if not os.path.exists(graph):
        rng = random.Random(n * 31 + len(pattern))
        rec = np.dtype([("pos", "<u4"), ("id", "<i8")])
        parts, text, at = [], [], 0
        for c, size in enumerate(sizes):
            if size is None:
                pos, cid = np.arange(abundance, dtype=np.int64), np.full(abundance, empty_id, dtype=np.int64)
            else:
                pos, cid = _positions(size, c), vid[at:at + size]
                at += size
            block = np.zeros(len(pos) + 1, dtype=rec)
            block["pos"][:-1], block["id"][:-1] = pos, cid
            block["pos"][-1], block["id"][-1] = SEP
            parts.append(block)
            text.append(">c%d\n%s\n" % (c, "".join(rng.choice("ACGT") for _ in range(int(pos[-1]) + K + 2))))
        assert at == n
        with open(fasta, "w") as f:
            f.write("".join(text))
        np.concatenate(parts).tofile(graph)
    return dict(graph=graph, fasta=fasta, k=K, a=abundance, positions=n, vertices=empty_id + 1, empty_chr=sizes.index(None), chromosomes=len(sizes))


def all_filtered(tmp, a=5):
    """Two chromosomes of `a` records of one vertex at abundance `a`: the filter drops every record, P = 0. (edge_inputs' all_filtered keeps
    the junctions that occur once.) -> dict(graph, fasta, k, a)."""
    graph, fasta = os.path.join(str(tmp), "table_all_filtered.bin"), os.path.join(str(tmp), "table_all_filtered.fa")
    if not os.path.exists(graph):
        rng = random.Random(77)
        block = np.zeros(a + 1, dtype=np.dtype([("pos", "<u4"), ("id", "<i8")]))
        block["pos"][:-1], block["id"][:-1] = np.arange(a) * 3, 9
        block["pos"][-1], block["id"][-1] = SEP
        with open(fasta, "w") as f:
            f.write("".join(">c%d\n%s\n" % (c, "".join(rng.choice("ACGT") for _ in range(3 * a + K + 2))) for c in range(2)))
        np.concatenate([block, block]).tofile(graph)
    return dict(graph=graph, fasta=fasta, k=K, a=a)


def expected_passes(pattern, n):
    """(sort passes, skipped) of the 4-digit key for the pattern, where it is known by construction; else None."""
    if pattern == "one_vertex":
        return 0, 4
    if pattern == "high_byte":
        return 1, 3
    return None
