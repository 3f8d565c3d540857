#!/usr/bin/env python3
"""Same-box A/B of the two routes to a device's tables on one input: the host route (createTables of csrc/device.hip: look-ahead
windows and occurrence records made by host threads, about 30 B per occurrence uploaded - its code is the parent commit's: the
baseline) against the device route (csrc/tables.hip: 10 B per occurrence uploaded, the rest computed by HIP kernels).

    python scripts/tables_ab.py <graph> <fasta> <k> <abundance> [--rounds 5] [--threads 16] [--limit 900] [--b 200]

One untimed creation of each first, then `--rounds` rounds of: create a host-route device, create a device-route device, read every
table of both back and compare them byte for byte (the first difference ends the run with status 1), destroy both. Printed per round:
wall clock of both creations (the whole lcb_device_create_tables call: tables, `used` bitmap, workspaces, lanes) and lcb_table_stats of
both - upload_ms is the wall time of the synchronous H2D copies, the device phases are hipEvent-timed; at the end medians and
max - min. "other" is what a creation spends outside the table step's copies and kernels: on the host route that includes the host
computation of the windows and records, on both the allocations and everything after the tables.

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

PHASES = ("upload_ms", "window_ms", "csr_ms", "sort_ms", "gather_ms")


def worker(args):
    import sibeliaz_amd
    from sibeliaz_amd import api
    t = time.time()
    st = sibeliaz_amd.JunctionStorage(args.graph, [args.fasta], args.k, threads=args.threads, abundance=args.abundance)
    print("input: %d positions, %d vertices, %d chromosomes; loaded in %.2f s" % (st.n_positions(), st.GetVerticesNumber(), st.GetChrNumber(), time.time() - t), flush=True)
    p = sibeliaz_amd.Params.make(args.k, b=args.b, m=50)

    def create(route):
        t0 = time.time()
        d = sibeliaz_amd.Device(st, p, 0, tables=route)
        return d, 1000 * (time.time() - t0)

    def equal(host, dev):
        for name in sorted(api.TABLES):
            if host.read_table(name).tobytes() != dev.read_table(name).tobytes():
                print("DIFFERENT: table %s" % name, flush=True)
                return False
        return True

    rows = []
    for r in range(-1, args.rounds):                  # round -1 is untimed
        host, t_host = create("host")
        dev, t_dev = create("device")
        hs, ds = host.table_stats, dev.table_stats
        ok = equal(host, dev)
        host.close()
        dev.close()
        if not ok:
            return 1
        if r < 0:
            print("tables equal; H2D bytes host route %d, device route %d; sort passes %d (+%d skipped); peak of the build's temporaries %d B (%.2f B per position)" % (
                hs["upload_bytes"], ds["upload_bytes"], ds["sort_passes"], ds["sort_passes_skipped"], ds["device_bytes"], ds["device_bytes"] / max(1, ds["positions"])), flush=True)
            continue
        dphase = sum(ds[k] for k in PHASES)
        rows.append((t_host, hs["upload_ms"], t_host - hs["upload_ms"], t_dev) + tuple(ds[k] for k in PHASES) + (t_dev - dphase,))
        print("round %d: host route %.1f ms = upload %.1f + other %.1f | device route %.1f ms = upload %.1f + window %.2f + csr %.2f + sort %.2f + gather %.2f + other %.1f" % ((r,) + rows[-1]), flush=True)
    names = ("host route", "host upload", "host other", "device route", "dev upload", "dev window", "dev csr", "dev sort", "dev gather", "dev other")
    for i, n in enumerate(names):
        col = [row[i] for row in rows]
        print("%-12s median %.2f ms, min %.2f, max %.2f (max - min %.2f)" % (n, statistics.median(col), min(col), max(col), max(col) - min(col)), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("graph")
    ap.add_argument("fasta")
    ap.add_argument("k", type=int)
    ap.add_argument("abundance", type=int)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--b", type=int, default=200, help="maxBranchSize (the look-ahead windows depend on it)")
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), args.graph, args.fasta, str(args.k), str(args.abundance),
           "--rounds", str(args.rounds), "--threads", str(args.threads), "--b", str(args.b), "--worker"]
    rc = subprocess.call(cmd)
    if rc:
        print("tables_ab: the measuring process ended with status %d" % rc, flush=True)
    sys.exit(rc)


if __name__ == "__main__":
    main()
