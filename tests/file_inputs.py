"""Hand-packed junction files for the tests of the junction file opened on the GPU (emulator, sanitizer program and MI355X): what no
lcb-mkgraph output has - ids with the sign set or with high bits, separators of either kind, none or several at the end, stray bytes,
sparse ids, filtered records that lie anywhere - and one defect each for the refusals. A record is struct.pack('<Iq', pos, id); the
FASTA next to a file is random bases of the right lengths. Data, generated at test time.

Sized for tiles of TILE = 64 records: a few hundred to a few thousand records each; `tile_edges` has a separator as the last record of
a tile, one as the first record of a tile, and a tile of separators only."""
import os
import random
import struct
import zlib

TILE = 64
K = 15
INT64_MAX = (1 << 63) - 1
SEP_POS = (0xFFFFFFFF, 5)               # a separator by its position alone
SEP_ID = (123, INT64_MAX)               # ... by its id alone
SEP_BOTH = (0xFFFFFFFF, INT64_MAX)      # ... as the tools write it

LEGAL = ["signed_ids", "high_bits", "separators_either_way", "no_trailing_separator", "three_trailing_separators", "stray_bytes", "sparse_ids",
         "long_chromosome", "all_filtered", "filtered_beyond_end", "tile_edges", "separators_only", "empty"]
ERRORS = {
    "err_empty_run": "the junction file has a chromosome without junctions (unsupported)",
    "err_unordered": "junction positions must strictly increase within a chromosome",
    "err_beyond_end": "a junction lies beyond the end of its sequence (junction file and FASTA do not match)",
    "err_fasta_more": "the FASTA input has more records than the junction file has chromosomes",
    "err_fasta_fewer": "the FASTA input has fewer records than the junction file has chromosomes",
}
NAMES = LEGAL + list(ERRORS)


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _chromosome(rng, n, length, ids):
    """n records at ascending positions that leave room for a k-mer, ids drawn by ids()."""
    return [(p, ids()) for p in sorted(rng.sample(range(length - K + 1), n))]


def build(name, tmp):
    """-> dict(graph, fasta=[path], k, a, b, m, error=the loader's text or None, sizes=records per chromosome, separators=those in the file)."""
    rng = random.Random(zlib.crc32(name.encode()))
    a, trailing, stray = 150, 1, b""
    sizes, lengths = [200, 90, 310], [900, 400, 1300]
    sep = lambda c: SEP_BOTH
    ids = lambda: rng.randint(1, 120) * rng.choice((1, -1))
    if name == "sparse_ids":                      # the largest id is ten times the number of distinct ones
        pool = [10 * j for j in range(1, 51)]
        ids = lambda: rng.choice(pool) * rng.choice((1, -1))
    elif name == "long_chromosome":               # more than 20 tiles in one chromosome
        sizes, lengths = [100, 1500, 80], [500, 4000, 300]
    elif name == "tile_edges":
        sizes, lengths, trailing = [63, 64, 63], [300, 300, 300], TILE + 3
    elif name in ("all_filtered", "filtered_beyond_end"):
        serial = iter(range(2, 1 << 20))          # every id exactly twice
        ids = lambda: next(serial) // 2 * rng.choice((1, -1))
        a = 2 if name == "all_filtered" else 4
    elif name == "separators_either_way":
        sep = lambda c: (SEP_POS, SEP_ID, SEP_BOTH)[c % 3]
    elif name == "no_trailing_separator":
        trailing = 0
    elif name == "three_trailing_separators":
        trailing = 3
    elif name == "stray_bytes":
        stray = b"\x01\x02\x03\x04\x05"
    if name in ("empty", "separators_only"):
        sizes, lengths, trailing = [], [], 0 if name == "empty" else 5
    chrs = [_chromosome(rng, n, length, ids) for n, length in zip(sizes, lengths)]
    if name == "sparse_ids":
        chrs[0][0] = (chrs[0][0][0], 500)
    if name == "filtered_beyond_end":             # id 9000 occurs four times: filtered; two of them lie where no kept record may
        chrs[0] += [(5, 9000), (2, -9000)]
        chrs[1] += [(lengths[1] + 1000, 9000), (0xFFFFFFFE, -9000)]
    if name == "high_bits":                       # bits above the low 32 that the cut to int32_t drops
        chrs = [[(p, (i & 0xFFFFFFFF) | (rng.randint(1, 0x7FFFFFFE) << 32)) for p, i in ch] for ch in chrs]
    if name == "err_unordered":
        chrs[1][40], chrs[1][41] = chrs[1][41], chrs[1][40]
    if name == "err_beyond_end":
        chrs[1][-1] = (lengths[1] - K + 1, chrs[1][-1][1])
    recs, separators = [], 0
    for c, ch in enumerate(chrs):
        recs += ch
        if c + 1 < len(chrs) or trailing:
            recs.append(sep(c))
            separators += 1
            if name == "err_empty_run" and c == 0:
                recs.append(sep(c))
                separators += 1
    tail = max(0, trailing - 1) if chrs else trailing
    recs += [sep(len(chrs) + j) for j in range(tail)]
    separators += tail
    n_fasta = len(chrs) + (1 if name == "err_fasta_more" else -1 if name == "err_fasta_fewer" else 0)
    graph, fasta = os.path.join(str(tmp), name + ".bin"), os.path.join(str(tmp), name + ".fa")
    with open(graph, "wb") as f:
        f.write(b"".join(struct.pack("<Iq", p, i) for p, i in recs) + stray)
    with open(fasta, "w") as f:
        f.write("".join(">c%d\n%s\n" % (c, _seq(rng, (lengths + [200])[c])) for c in range(n_fasta)))
    return dict(graph=graph, fasta=[fasta], k=K, a=a, b=200, m=50, error=ERRORS.get(name), sizes=[len(ch) for ch in chrs], separators=separators)
