#!/usr/bin/env python3
"""Record what the command-line tool answers to every setting of its route switches: `make_cli_routes.py EXE OUT`.

EXE is a built sibeliaz-lcb - for the committed tests/golden/cli_routes.tsv the one of the commit before the routes became a list in
main.cpp -, OUT the file to write: one line per run of tests/cli_inputs.route_matrix(), with the settings, the exit status, stdout and
stderr. The inputs do not exist, so every run ends before any GPU work; record on a machine without a GPU (only there does
LCB_JUNCTIONS=device answer `no HIP device`, which tests/test_cli_routes_cpu.py then knows to skip where there is one)."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import cli_inputs  # noqa: E402


def main(exe, out):
    with ThreadPoolExecutor(8) as pool:
        lines = list(pool.map(lambda env: cli_inputs.route_run(env, exe), cli_inputs.route_matrix()))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d runs -> %s" % (len(lines), out))


if __name__ == "__main__":
    main(*sys.argv[1:3])
