#!/usr/bin/env python3
"""Generate tests/golden/edge_cases/<name>/ from the REAL reference: for every input of tests/edge_inputs.py, what the unmodified
reference binary (oracle/_ref/sibeliaz-lcb-ref, built by `make -C oracle ref`) writes - blocks_coords.gff, its two summary lines
(summary.txt) and, with --chunks 3, the block sequences (seq_<i>.txt = <i>.tmp). Only where oracle/_ref exists; what is committed
is its output, data only. tests/test_edge_cases.py compares the oracle and the product against these files."""
import os
import re
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import edge_inputs as E  # noqa: E402

OUT = os.path.join(HERE, "edge_cases")
CHUNKS = 3


def main():
    ref = os.path.join(ROOT, "oracle", "_ref", "sibeliaz-lcb-ref")
    if not os.path.exists(ref):
        raise SystemExit("needs oracle/_ref/sibeliaz-lcb-ref (make -C oracle ref)")
    tmp = tempfile.mkdtemp()
    try:
        for name in E.NAMES:
            case = E.build(name, tmp)
            r = E.run_cli(ref, case, os.path.join(tmp, name), ["--chunks", str(CHUNKS)])
            assert r.returncode == 0, r.stderr
            d = os.path.join(OUT, name)
            os.makedirs(d, exist_ok=True)
            shutil.copyfile(os.path.join(tmp, name, "blocks_coords.gff"), os.path.join(d, "blocks_coords.gff"))
            for i in range(CHUNKS):
                shutil.copyfile(os.path.join(tmp, name, "%d.tmp" % i), os.path.join(d, "seq_%d.txt" % i))
            with open(os.path.join(d, "summary.txt"), "w") as f:
                f.write("".join(x + "\n" for x in re.findall(r"^(Blocks found: .*|Coverage: .*)$", r.stdout, re.M)))
            print(name, "ok")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
