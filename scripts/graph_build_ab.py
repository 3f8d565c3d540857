#!/usr/bin/env python3
"""Same-box A/B of the two routes from FASTA files to a graph on one input: the two-step route (build_junctions writes the junction
file on the GPU, JunctionStorage reads it and the FASTA again: the parent commit's code, the baseline) against the device route
(JunctionStorage.build: lcb_graph_build, csrc/junctions.hip + lcb_graph_kernels.h, no file).

    python scripts/graph_build_ab.py <workload> [--rounds 5] [--threads 16] [--limit 900] [--abundance-ab]

<workload> is a name of bench.WORKLOADS (ecoli62: k = 15; mice16_scaled: k = 25; made by bench.ensure_workload), or heavy:<copies>: the
repeat-heavy input of tests/seed_inputs.py (one 60-base repeat, <copies> copies on both strands in 50 records, k = 15), where every
lane of the abundance kernel hits the same few counters.

One untimed round of each route first - there all nine tables of a device made of either graph are compared as well -, then `--rounds`
rounds of: the two-step route, the device route, the two graphs compared byte for byte (chromosomes, names, lengths, chr_start, pos_id,
pos_pos, vertices, and the host enumerator's seeds, which are made of posCh and the CSR); the first difference ends the run with status
1. Printed per round: the wall clock of both routes and their parts (junction file / load; the phases of lcb_graph_build_stats); at the
end median (min .. max) of each. --abundance-ab: every round builds twice more, with LCB_GRAPH_ABUNDANCE=plain and =wave, and reports
abundance_ms of both (the kernel alone, hipEvent-timed).

The measurement runs in a child process under `timeout -k 10 <limit>`, so a device step that hangs ends the run instead of holding
the GPU; the parent only reports the child's status."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("parse_ms", "upload_ms", "insert_ms", "mark_ms", "count_ms", "emit_ms", "take_ms", "abundance_ms", "compact_ms", "download_ms", "csr_ms")


def the_input(name):
    if name.startswith("heavy:"):
        from tests import seed_inputs
        copies = int(name.split(":")[1])
        d = os.path.join(os.environ.get("LCB_BENCH_DIR", "/tmp/lcb_bench"), "heavy_%d" % copies)
        os.makedirs(d, exist_ok=True)
        fa = os.path.join(d, "genomes.fa")
        if not os.path.exists(fa):
            with open(fa + ".tmp", "w") as f:
                f.write(seed_inputs.heavy_text(copies, 50, 3, 0))
            os.rename(fa + ".tmp", fa)
        return dict(fasta=fa, k=seed_inputs.K, a=150)
    import bench
    return bench.ensure_workload(name)


def same(a, b, threads, tables):
    import sibeliaz_amd
    from sibeliaz_amd import api
    if a.GetChrNumber() != b.GetChrNumber() or a.GetVerticesNumber() != b.GetVerticesNumber():
        return "chromosomes / vertices"
    for c in range(a.GetChrNumber()):
        if a.GetChrDescription(c) != b.GetChrDescription(c) or a.chr_len(c) != b.chr_len(c):
            return "name / length of chromosome %d" % c
    for what in ("chr_start", "pos_id", "pos_pos"):
        if getattr(a, what)().tobytes() != getattr(b, what)().tobytes():
            return what
    if a.seeds(threads).tobytes() != b.seeds(threads).tobytes():
        return "seeds"
    if tables:
        p = sibeliaz_amd.Params.make(a.k)
        da, db = sibeliaz_amd.Device(a, p, 0), sibeliaz_amd.Device(b, p, 0)
        try:
            for name in sorted(api.TABLES):
                if da.read_table(name).tobytes() != db.read_table(name).tobytes():
                    return "device table " + name
        finally:
            da.close()
            db.close()
    return None


def worker(args):
    import sibeliaz_amd
    w = the_input(args.workload)
    fa, k, a = w["fasta"], w["k"], w["a"]
    print("input: %s, %d bytes of FASTA, k = %d, abundance = %d, %d host threads" % (args.workload, os.path.getsize(fa), k, a, args.threads), flush=True)
    rows, ab = [], []
    with tempfile.TemporaryDirectory() as tmp:
        jf = os.path.join(tmp, "junctions.bin")
        for r in range(-1, args.rounds):                  # round -1 is untimed
            t0 = time.time()
            js = sibeliaz_amd.build_junctions([fa], k, jf)
            t1 = time.time()
            two = sibeliaz_amd.JunctionStorage(jf, [fa], k, threads=args.threads, abundance=a)
            t2 = time.time()
            dev, ds = sibeliaz_amd.JunctionStorage.build([fa], k, abundance=a, threads=args.threads, stats=True)
            t3 = time.time()
            diff = same(two, dev, args.threads, tables=r < 0)
            file_bytes = os.path.getsize(jf)
            os.remove(jf)
            two.close()
            dev.close()
            if diff:
                print("DIFFERENT: %s" % diff, flush=True)
                return 1
            if args.abundance_ab:
                pair = []
                for mode in ("plain", "wave"):
                    os.environ["LCB_GRAPH_ABUNDANCE"] = mode
                    st, s = sibeliaz_amd.JunctionStorage.build([fa], k, abundance=a, threads=args.threads, stats=True)
                    st.close()
                    pair.append(s["abundance_ms"])
                del os.environ["LCB_GRAPH_ABUNDANCE"]
                if r >= 0:
                    ab.append(tuple(pair))
            if r < 0:
                print("graphs equal (device tables too); raw %d, kept %d, vertices %d, patched %d; junction file %d B, downloaded %d B, peak device memory %d B" % (
                    ds["raw_occurrences"], ds["kept_occurrences"], ds["vertices"], ds["patched"], file_bytes, ds["download_bytes"], ds["peak_device_bytes"]), flush=True)
                continue
            row = (1000 * (t2 - t0), 1000 * (t1 - t0), js["read_ms"], js["write_ms"], 1000 * (t2 - t1), 1000 * (t3 - t2)) + tuple(ds[p] for p in PHASES)
            rows.append(row)
            print("round %d: two-step %.0f ms = junction file %.0f (read %.0f, write %.0f) + load %.0f | device route %.0f ms: " % ((r,) + row[:6])
                  + " ".join("%s %.1f" % (p[:-3], ds[p]) for p in PHASES), flush=True)
    names = ("two-step route", "  junction file", "    its read", "    its write", "  load", "device route") + tuple("  " + p for p in PHASES)
    for i, n in enumerate(names):
        col = [row[i] for row in rows]
        print("%-16s median %.1f ms (%.1f .. %.1f)" % (n, statistics.median(col), min(col), max(col)), flush=True)
    for i, n in enumerate(("abundance plain", "abundance wave") if ab else ()):
        col = [x[i] for x in ab]
        print("%-16s median %.3f ms (%.3f .. %.3f)" % (n, statistics.median(col), min(col), max(col)), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--abundance-ab", action="store_true")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), args.workload, "--rounds", str(args.rounds), "--threads", str(args.threads), "--worker"]
    rc = subprocess.call(cmd + (["--abundance-ab"] if args.abundance_ab else []))
    if rc:
        print("graph_build_ab: the measuring process ended with status %d" % rc, flush=True)
    sys.exit(rc)


if __name__ == "__main__":
    main()
