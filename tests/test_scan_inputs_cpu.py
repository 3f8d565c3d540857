"""What keeps tests/test_gpu_scan_pieces.py from passing vacuously: the two inputs of tests/scan_inputs.py have, by the host route alone
(the JunctionStorage loader, the host seed enumerator, the CPU lcb-mkgraph), the sizes at which every one-workgroup scan of the device
routes takes at least three pieces, and the chromosome boundaries, emptied blocks and late patches they are meant to have. Every
condition is asserted exactly. No GPU."""
import os
import subprocess

import numpy as np
import pytest

import sibeliaz_amd
from tests import scan_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MKGRAPH = os.path.join(ROOT, "sibeliaz_amd", "bin", "lcb-mkgraph")
REC = np.dtype([("pos", "<u4"), ("id", "<i8")])
PIECE = 4096                 # entries of one piece of seedScan32, tableScan32/64 and graphScan
TILE = 1024                  # records per sort tile (S_TILE, T_TILE): 256 histogram entries each
WAVE_VERTICES = 32           # S_VPW: the vertices of one entry of seedScan64


def pieces(entries):
    return (entries + PIECE - 1) // PIECE


def split(path):
    """-> the non-separator records of a junction file, the file index of every separator."""
    data = np.fromfile(path, dtype=REC)
    sep = (data["pos"] == 0xFFFFFFFF) | (data["id"] == (1 << 63) - 1)
    return data[~sep], np.nonzero(sep)[0]


@pytest.fixture(scope="module")
def packed(built, tmp_path_factory):
    c = scan_inputs.packed(tmp_path_factory.mktemp("scan_packed"))
    st = sibeliaz_amd.JunctionStorage(c["graph"], c["fasta"], c["k"], threads=4, abundance=c["a"])
    yield c, st
    st.close()


def test_packed_file_has_the_raw_records_and_boundaries_it_promises(packed):
    c, st = packed
    raw, sep = split(c["graph"])
    N = scan_inputs.N
    assert len(raw) == N == 2 * (1 << 20) + 300 * 256 + 77
    assert os.path.getsize(c["graph"]) == 12 * (N + len(sep))
    first = np.concatenate([[0], sep[:-1] - np.arange(len(sep) - 1)])          # raw index of the first record of every chromosome
    assert len(sep) >= 7 and first.tolist() == scan_inputs.FIRST == c["first"]
    assert 4096 * 256 in first and 4096 * 256 - 1 in first
    on_block = [int(f) for f in first[1:] if f % 256 == 0]
    assert on_block == [4096 * 256], "a chromosome boundary other than the one meant falls on a block boundary"
    sizes = np.diff(np.concatenate([first, [N]]))
    assert sorted(np.nonzero(sizes == 1)[0].tolist()) == sorted(scan_inputs.SINGLE) and sizes[5] == 1 and first[6] == first[5] + 1
    # graphScan, at both call sites: three pieces, the last one partial
    for entries in ((N + len(sep) + 255) // 256, (N + 255) // 256):
        assert entries > 2 * PIECE and pieces(entries) == 3 and entries % PIECE != 0
    # positions ascend strictly inside every chromosome, in steps of 1 to 3
    pos = raw["pos"].astype(np.int64)
    inner = np.ones(N, dtype=bool)
    inner[first] = False
    step = np.diff(pos, prepend=0)[inner]
    assert step.min() == 1 and step.max() == 3
    assert os.path.getsize(c["fasta"][0]) < 2.2 * N


def test_packed_file_keeps_half_of_its_records_in_vertices_of_four(packed):
    c, st = packed
    raw, sep = split(c["graph"])
    N, P, V = scan_inputs.N, st.n_positions(), st.GetVerticesNumber()
    assert P == c["kept"] and V == c["vertices"]
    assert 0.3 < P / N < 0.7
    assert P > 2 * 16384 * 16              # the tile histograms of the table sort: 256 entries per 1024 positions
    assert pieces((P + TILE - 1) // TILE * 256) >= 3
    assert V > 3 * 32768                   # the wavefront slots of the seed count: a run of more than three entries per lane
    assert ((V + WAVE_VERTICES - 1) // WAVE_VERTICES + 1023) // 1024 >= 3
    assert V + 1 > 4096 * 16 and pieces(V + 1) >= 3                            # the vertex counters of the table build
    # every kept vertex exactly four times, about one occurrence in four with the sign set; the hot ids all dropped
    ids = st.pos_id().astype(np.int64)
    count = np.bincount(np.abs(ids), minlength=V)
    lo, hi = c["hot_ids"]
    assert (count[1:lo] == 4).all() and (count[lo:] == 0).all() and count[0] == 0 and hi + 1 == V
    assert 0.2 < (ids < 0).mean() < 0.3
    hot = np.bincount(np.abs(raw["id"]), minlength=V)[lo:]
    assert len(hot) == scan_inputs.HOT and (hot >= c["a"]).all() and (hot - c["a"]).max() < 50, "abundance is not just below the hot ids' counts"
    every_second = (np.abs(raw["id"]) >= lo)[1::2]
    assert every_second.mean() > 0.999
    # the scatter of the table sort is not local: the four occurrences of a vertex lie far apart
    order = np.argsort(np.abs(ids), kind="stable").reshape(-1, 4)
    assert np.median(order[:, 3] - order[:, 0]) > P // 4


def test_packed_file_has_its_emptied_blocks_and_late_patches(packed):
    c, st = packed
    raw, sep = split(c["graph"])
    cs = st.chr_start().astype(np.int64)
    e = scan_inputs.EMPTIED
    assert st.GetChrNumber() == len(scan_inputs.FIRST) >= 7
    assert cs[e + 1] == cs[e], "the abundance filter does not empty chromosome %d" % e
    sizes = np.diff(cs)
    assert (np.delete(sizes, e) > 0).all() and sizes[scan_inputs.SINGLE[0]] == sizes[scan_inputs.SINGLE[1]] == 1
    lo, hi = scan_inputs.FIRST[e], scan_inputs.FIRST[e + 1]
    assert (hi // 256) - ((lo + 255) // 256) >= 2, "the emptied chromosome spans fewer than two whole blocks of raw records"
    assert (np.abs(raw["id"][lo:hi]) >= c["hot_ids"][0]).all()
    # the characters the device cannot code: behind the k-mer of kept records with a kept index beyond 2^20
    text = open(c["fasta"][0], "rb").read().split(b"\n")
    seqs = [np.frombuffer(s, dtype=np.uint8) for s in text[1::2] if s]
    assert len(seqs) == st.GetChrNumber() and [len(s) for s in seqs] == [st.chr_len(i) for i in range(len(seqs))]
    pos = st.pos_pos().astype(np.int64)
    late = 0
    for ch in range(len(seqs)):
        q = np.arange(cs[ch], cs[ch + 1])
        n_at = seqs[ch][pos[q] + c["k"]] == ord("n")
        late += int((n_at & (q > 1 << 20)).sum())
    assert late == c["patched"] >= 24, "only %d kept records beyond index 2^20 have a lower-case n behind their k-mer" % late
    assert sum(int((s == ord("n")).sum()) for s in seqs) == c["patched"]


def test_packed_file_gives_seeds_for_three_pieces_of_the_seed_sort(packed):
    c, st = packed
    seeds = st.seeds(4)
    assert len(seeds) > 3 * 16384
    assert pieces((len(seeds) + TILE - 1) // TILE * 256) >= 3
    assert int(seeds["count"].max()) <= 4


def test_fasta_has_a_tile_of_three_blocks_per_lane_and_blocks_without_junctions(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_copies")
    c = scan_inputs.fasta(tmp)
    text = open(c["fasta"][0], "rb").read().split(b"\n")
    assert len(text) == 3 and text[2] == b"" and text[0].startswith(b">")
    windows = len(text[1]) - c["k"] + 1
    assert windows == c["windows"] >= 700001
    code_len = len(text[1]) + 2                       # a breaker in front of the record and one behind it: the windows of the tile loop
    nb = (code_len + 255) // 256
    assert nb == 2735 and (nb + 1023) // 1024 == 3
    assert [(min(300000, code_len - t) + 255) // 256 for t in range(0, code_len, 300000)] == [1172, 1172, 391]      # per = 2, 2, 1
    graph = str(tmp / "copies.bin")
    subprocess.check_call([MKGRAPH, "-k", str(c["k"]), "-o", graph] + c["fasta"], stderr=subprocess.DEVNULL)
    raw, sep = split(graph)
    assert len(sep) == 1 and len(raw) > 256
    # block b of the default tile holds the windows at code positions [256 b, 256 b + 256), window g = base 1 + its position
    per_block = np.bincount((raw["pos"].astype(np.int64) + 1) // 256, minlength=nb)
    lo, hi = c["stretch"]
    inside = np.arange((lo + 1 + 255) // 256, (hi - c["k"] + 1) // 256)          # blocks whose windows lie in the stretch entirely
    assert len(inside) > 200
    assert (per_block[inside] == 0).sum() >= 1, "every block of the unrelated stretch has a junction"
    assert (per_block > 0).sum() > 1024, "fewer than 1024 blocks have junctions"
