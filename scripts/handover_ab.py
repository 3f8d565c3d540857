#!/usr/bin/env python3
"""Same-box A/B of the two routes from FASTA files to a graph and a ready device on one input: the composed route (JunctionStorage.build
= lcb_graph_build, then Device(..., tables="device") = lcb_device_create_tables(LCB_TABLES_DEVICE): the parent commit's code, the
baseline) against the hand-over route (open_fasta = lcb_open_fasta).

    python scripts/handover_ab.py <workload> [--rounds 5] [--threads 16] [--limit 900]

<workload> is a name of bench.WORKLOADS (ecoli62: k = 15; mice16_scaled: k = 25; made by bench.ensure_workload) or heavy:<copies> (the
repeat-heavy input of tests/seed_inputs.py in 50 records, k = 15).

One untimed round first, then `--rounds` rounds; every round runs both routes in one process, the composed route first in even rounds
and second in odd ones, and compares the two results: the graph (chromosomes, names, lengths, chr_start, pos_id, pos_pos, vertices, the
host enumerator's seeds, which are made of posCh and the host CSR) and all nine tables of the two devices. The first difference ends the
run with status 1. Printed per round: the wall clock of both routes and the phases of the new one; at the end median (min .. max).

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



def the_input(name):
    """-> dict(fasta, k, a, b, m). Only the FASTA is made: neither route reads a junction file."""
    if name.startswith("heavy:"):
        from scripts.graph_build_ab import the_input as heavy_input
        return heavy_input(name)
    import bench
    w = bench.WORKLOADS[name]
    d = os.path.join(os.environ.get("LCB_BENCH_DIR", "/tmp/lcb_bench"), w.get("files", name) + "_fasta")
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "genomes.fa")
    if not os.path.exists(fa):
        t = time.time()
        subprocess.check_call([os.path.join(bench.BIN, "lcb-synth"), "-o", fa + ".tmp"] + w["synth"].split())
        os.rename(fa + ".tmp", fa)
        print("generated %s in %.1f s" % (name, time.time() - t), flush=True)
    return dict(w, fasta=fa)


OLD = ("build_ms", "  parse_ms", "  download_ms", "  csr_ms", "tables_ms", "  upload_ms")
NEW = ("parse_ms", "upload_ms", "insert_ms", "count_ms", "emit_ms", "take_ms", "abundance_ms", "compact_ms", "place_ms", "download_ms", "patch_ms", "window_ms", "table_csr_ms", "sort_ms",
       "csr_download_ms", "gather_ms")


def same(a, da, b, db, threads):
    import numpy as np
    from sibeliaz_amd import api
    if a.GetChrNumber() != b.GetChrNumber() or a.GetVerticesNumber() != b.GetVerticesNumber():
        return "chromosomes / vertices"
    for c in range(a.GetChrNumber()):
        if a.GetChrDescription(c) != b.GetChrDescription(c) or a.chr_len(c) != b.chr_len(c):
            return "name / length of chromosome %d" % c
    for what in ("chr_start", "pos_id", "pos_pos"):
        if not np.array_equal(getattr(a, what)(), getattr(b, what)()):
            return what
    if not np.array_equal(a.seeds(threads), b.seeds(threads)):
        return "seeds"
    for name in sorted(api.TABLES):
        if not np.array_equal(da.read_table(name), db.read_table(name)):
            return "device table " + name
    return None


def worker(args):
    import sibeliaz_amd
    w = the_input(args.workload)
    fa, k, a = w["fasta"], w["k"], w["a"]
    p = sibeliaz_amd.Params.make(k, b=w.get("b", 200), m=w.get("m", 50))
    print("input: %s, %d bytes of FASTA, k = %d, abundance = %d, %d host threads" % (args.workload, os.path.getsize(fa), k, a, args.threads), flush=True)
    rows = []

    def composed():
        t0 = time.time()
        st, gs = sibeliaz_amd.JunctionStorage.build([fa], k, abundance=a, threads=args.threads, stats=True)
        t1 = time.time()
        dev = sibeliaz_amd.Device(st, p, 0, tables="device")
        t2 = time.time()
        return st, dev, (1000 * (t2 - t0), 1000 * (t1 - t0), gs["parse_ms"], gs["download_ms"], gs["csr_ms"], 1000 * (t2 - t1), dev.table_stats["upload_ms"])

    def handover():
        t0 = time.time()
        st, dev, s = sibeliaz_amd.open_fasta([fa], k, p, abundance=a, threads=args.threads, stats=True)
        return st, dev, (1000 * (time.time() - t0),) + tuple(s[n] for n in NEW), s

    for r in range(-1, args.rounds):                      # round -1 is untimed
        if r % 2 == 0:
            old, new = composed(), handover()
        else:
            new = handover()
            old = composed()
        diff = same(old[0], old[1], new[0], new[1], args.threads)
        s = new[3]
        for st, dev in (old[:2], new[:2]):
            dev.close()
            st.close()
        if diff:
            print("DIFFERENT: %s" % diff, flush=True)
            return 1
        if r < 0:
            print("graphs and all nine device tables equal; kept %d, vertices %d, patched %d; downloaded %d B + CSR %d B, table step uploaded %d B, peak device memory %d B" % (
                s["kept_occurrences"], s["vertices"], s["patched"], s["download_bytes"], s["csr_download_bytes"], s["upload_bytes"], s["peak_device_bytes"]), flush=True)
            continue
        rows.append(old[2] + new[2])
        print("round %d: composed %.0f ms = build %.0f (parse %.0f, download %.0f, csr %.0f) + tables %.0f (upload %.0f) | hand-over %.0f ms: " % ((r,) + old[2] + new[2][:1])
              + " ".join("%s %.1f" % (n[:-3], v) for n, v in zip(NEW, new[2][1:])), flush=True)
    names = ("composed route",) + tuple("  " + n for n in OLD) + ("hand-over route",) + tuple("  " + n for n in NEW)
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
        print("handover_ab: the measuring process ended with status %d" % rc, flush=True)
    sys.exit(rc)


if __name__ == "__main__":
    main()
