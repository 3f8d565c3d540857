#!/usr/bin/env python3
"""Same-box A/B of the two routes from a junction file and its FASTA files to a graph and a ready device on one input: the composed
route (JunctionStorage(file, ...) = lcb_graph_load on host threads, then Device(..., tables="device") =
lcb_device_create_tables(LCB_TABLES_DEVICE): the parent commit's code, the yardstick) against open_junctions (= lcb_open_junctions,
DESIGN.md §15).

    python scripts/file_open_ab.py <workload> [--rounds 5] [--threads 16] [--limit 900]

<workload> is a name of bench.WORKLOADS (ecoli62: k = 15; mice16_scaled: k = 25; FASTA and junction file made by bench.ensure_workload,
the file by the CPU lcb-mkgraph).

One untimed round first, then `--rounds` rounds; every round runs both routes in one process, the composed route first in even rounds
and second in odd ones, and compares the two results: the graph (chromosomes, names, lengths, chr_start, pos_id, pos_pos, vertices, the
host enumerator's seeds, which are made of posCh and the host CSR) and all nine tables of the two devices. The first difference ends the
run with status 1. Printed per round: the wall clock of both routes and the phases of the new one; at the end median (min .. max) and
the bytes moved each way.

The measurement runs in a child process under `timeout -k 10 <limit>`, so a device step that hangs ends the run instead of holding
the GPU; the parent only reports the child's status."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.handover_ab import same  # noqa: E402  (the comparison of two (storage, device) pairs)

OLD = ("load_ms", "tables_ms", "  upload_ms")
NEW = ("read_ms", "upload_ms", "take_ms", "parse_ms", "abundance_ms", "compact_ms", "place_ms", "download_ms", "patch_ms", "window_ms", "table_csr_ms", "sort_ms", "csr_download_ms", "gather_ms")


def worker(args):
    import bench
    import sibeliaz_amd
    w = bench.ensure_workload(args.workload)
    gr, fa, k, a = w["graph"], w["fasta"], w["k"], w["a"]
    p = sibeliaz_amd.Params.make(k, b=w.get("b", 200), m=w.get("m", 50))
    print("input: %s, %d bytes of junction file, %d bytes of FASTA, k = %d, abundance = %d, %d host threads" % (args.workload, os.path.getsize(gr), os.path.getsize(fa), k, a, args.threads),
          flush=True)
    rows = []

    def composed():
        t0 = time.time()
        st = sibeliaz_amd.JunctionStorage(gr, [fa], k, threads=args.threads, abundance=a)
        t1 = time.time()
        dev = sibeliaz_amd.Device(st, p, 0, tables="device")
        t2 = time.time()
        return st, dev, (1000 * (t2 - t0), 1000 * (t1 - t0), 1000 * (t2 - t1), dev.table_stats["upload_ms"]), dev.table_stats

    def opened():
        t0 = time.time()
        st, dev, s = sibeliaz_amd.open_junctions(gr, [fa], k, p, abundance=a, threads=args.threads, stats=True)
        return st, dev, (1000 * (time.time() - t0),) + tuple(s[n] for n in NEW), s

    for r in range(-1, args.rounds):                      # round -1 is untimed
        if r % 2 == 0:
            old, new = composed(), opened()
        else:
            new = opened()
            old = composed()
        diff = same(old[0], old[1], new[0], new[1], args.threads)
        s, ts = new[3], old[3]
        chromosomes = new[0].GetChrNumber()
        codes = 1 + sum(new[0].chr_len(c) + 1 for c in range(chromosomes))          # one byte per base, a breaker around every record
        for st, dev in (old[:2], new[:2]):
            dev.close()
            st.close()
        if diff:
            print("DIFFERENT: %s" % diff, flush=True)
            return 1
        if r < 0:
            kept = s["kept_occurrences"]
            print("graphs and all nine device tables equal; chromosomes %d, raw %d, kept %d, vertices %d, patched %d, tiles %d" % (
                s["records"], s["raw_occurrences"], kept, s["vertices"], s["patched"], s["tiles"]), flush=True)
            print("bytes, composed route: host -> device %d (the table step; the file and the FASTA stay on the host), device -> host 0" % ts["upload_bytes"], flush=True)
            print("bytes, open_junctions: host -> device %d (file) + %d (code bytes and record bases) + %d (table step), device -> host %d + CSR %d; peak device memory %d" % (
                12 * (os.path.getsize(gr) // 12), codes + 8 * (chromosomes + 1), s["upload_bytes"], s["download_bytes"], s["csr_download_bytes"],
                s["peak_device_bytes"]), flush=True)
            continue
        rows.append(old[2] + new[2])
        print("round %d: composed %.0f ms = load %.0f + tables %.0f (upload %.0f) | open_junctions %.0f ms: " % ((r,) + old[2] + new[2][:1])
              + " ".join("%s %.1f" % (n[:-3], v) for n, v in zip(NEW, new[2][1:])), flush=True)
    names = ("composed route",) + tuple("  " + n for n in OLD) + ("open_junctions",) + tuple("  " + n for n in NEW)
    for i, n in enumerate(names):
        col = [row[i] for row in rows]
        print("%-20s median %.1f ms (%.1f .. %.1f)" % (n, statistics.median(col), min(col), max(col)), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), args.workload, "--rounds", str(args.rounds), "--threads", str(args.threads), "--worker"]
    rc = subprocess.call(cmd)
    if rc:
        print("file_open_ab: the measuring process ended with status %d" % rc, flush=True)
    sys.exit(rc)


if __name__ == "__main__":
    main()
