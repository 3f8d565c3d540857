#!/usr/bin/env python3
"""Same-box A/B of the two seed enumerators on one input: the host enumerator (csrc/bundles.cpp, OpenMP, 16 threads - its code is the
parent commit's, this change does not touch it: the baseline) against lcb_device_enumerate_seeds (csrc/seeds.hip) on the tables of a
device created once.

    python scripts/seed_enum_ab.py <graph> <fasta> <k> <abundance> [--rounds 5] [--threads 16] [--limit 900]

One untimed call of each first, then `--rounds` rounds of: host, device. Every round the two arrays are compared byte for byte; the
first difference ends the run with status 1. Printed per round: wall clock of both calls and the device call's lcb_seed_stats phases
(count / fill / sort are hipEvent-timed, copy is the D2H copy plus the expansion to lcb_seed on the host); at the end medians and
max - min of both. "rest" is what the device call spends outside its phases: hipMalloc / hipFree, and the binding's copy of the result
into a numpy array, which the host call pays as well (a plain copy of the result is timed next to it as a yardstick).

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


def worker(args):
    import sibeliaz_amd
    t = time.time()
    st = sibeliaz_amd.JunctionStorage(args.graph, [args.fasta], args.k, threads=args.threads, abundance=args.abundance)
    t_load = time.time() - t
    t = time.time()
    dev = sibeliaz_amd.Device(st, sibeliaz_amd.Params.make(args.k, b=200, m=50), 0)
    print("input: %d positions, %d vertices; loaded in %.2f s, device + tables in %.2f s" % (st.n_positions(), st.GetVerticesNumber(), t_load, time.time() - t), flush=True)
    host = st.seeds(args.threads)                     # untimed
    got, stats = dev.enumerate_seeds(stats=True)      # untimed
    if got.tobytes() != host.tobytes():
        print("DIFFERENT: the untimed device call does not give the host's seeds", flush=True)
        return 1
    print("seeds %d, largest count %d, sort passes %d (+%d skipped), device bytes %d" % (len(host), stats["max_count"], stats["sort_passes"], stats["sort_passes_skipped"],
                                                                                        stats["device_bytes"]), flush=True)
    rows = []
    for r in range(args.rounds):
        t = time.time()
        host = st.seeds(args.threads)
        t_host = time.time() - t
        t = time.time()
        got, s = dev.enumerate_seeds(stats=True)
        t_dev = time.time() - t
        if got.tobytes() != host.tobytes():
            print("DIFFERENT in round %d" % r, flush=True)
            return 1
        t = time.time()
        got.copy()                                    # what the binding adds to BOTH calls: one copy of the result into a fresh numpy array
        t_np = time.time() - t
        rows.append((1000 * t_host, 1000 * t_dev, s["count_ms"], s["fill_ms"], s["sort_ms"], s["copy_ms"], 1000 * t_np))
        print("round %d: host(%d threads) %.1f ms | device call %.1f ms = count %.2f + fill %.2f + sort %.2f + copy %.1f + rest %.1f | a numpy copy of the result %.1f ms" % (
            (r, args.threads) + rows[-1][:6] + (rows[-1][1] - sum(rows[-1][2:6]), rows[-1][6])), flush=True)
    names = ("host", "device call", "count", "fill", "sort", "copy", "numpy copy")
    for i, n in enumerate(names):
        col = [row[i] for row in rows]
        print("%-12s median %.2f ms, min %.2f, max %.2f (max - min %.2f)" % (n, statistics.median(col), min(col), max(col), max(col) - min(col)), flush=True)
    dev.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graph")
    ap.add_argument("fasta")
    ap.add_argument("k", type=int)
    ap.add_argument("abundance", type=int)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), args.graph, args.fasta, str(args.k), str(args.abundance),
           "--rounds", str(args.rounds), "--threads", str(args.threads), "--worker"]
    rc = subprocess.call(cmd)
    if rc:
        print("seed_enum_ab: the measuring process ended with status %d" % rc, flush=True)
    sys.exit(rc)


if __name__ == "__main__":
    main()
