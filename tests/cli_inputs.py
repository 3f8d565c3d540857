"""What the CPU tests of the command-line tool share: the environment switches that choose its routes, a run of the built executable
with all of them scrubbed, a run that must be refused before anything is loaded, and the matrix of switch settings whose outcome
tests/golden/cli_routes.tsv records (written by tests/golden/make_cli_routes.py, compared by tests/test_cli_routes_cpu.py)."""
import itertools
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sibeliaz_amd", "bin", "sibeliaz-lcb")
SWITCHES = ("LCB_LOAD", "LCB_HANDOVER", "LCB_JUNCTIONS", "LCB_TABLES", "LCB_SEEDS", "LCB_GPUS")
ROUTES_TSV = os.path.join(ROOT, "tests", "golden", "cli_routes.tsv")
TMP_TOKEN = "<TMP>"


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def cli(graph, fasta, out, args=("-k", "15"), exe=EXE, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    return subprocess.run([exe, "--graph", graph, fasta] + list(args) + ["-o", str(out)], capture_output=True, text=True, env=e)


def refused(tmp_path, line, **env):
    out = tmp_path / "out"
    r = cli(str(tmp_path / "no.bin"), str(tmp_path / "no.fa"), out, **env)
    assert r.returncode == 1 and r.stderr == line + "\n", r.stderr
    assert r.stdout == "" and not out.exists()


def route_matrix():
    """The settings of the route matrix, each a dict of the switches that are set: every combination of four route switches at unset, their
    values and an unknown one, with one GPU and two (216); LCB_SEEDS=x alone and with each other switch at x; each switch alone and empty."""
    axes = (("LCB_TABLES", (None, "host", "device", "x")), ("LCB_JUNCTIONS", (None, "device", "x")), ("LCB_HANDOVER", (None, "device", "x")),
            ("LCB_LOAD", (None, "device", "x")), ("LCB_GPUS", (None, "2")))
    runs = [{n: v for (n, _), v in zip(axes, combo) if v is not None} for combo in itertools.product(*(values for _, values in axes))]
    runs.append({"LCB_SEEDS": "x"})
    runs += [{"LCB_SEEDS": "x", n: "x"} for n in SWITCHES if n != "LCB_SEEDS"]
    runs += [{n: ""} for n in SWITCHES]
    return runs


def route_run(env, exe=EXE):
    """One run of the matrix, on inputs that do not exist (it ends before any GPU work) -> its line of cli_routes.tsv: the settings, the
    exit status, stdout and stderr (as JSON strings), with the temporary directory replaced by a fixed token."""
    with tempfile.TemporaryDirectory() as tmp:
        r = cli(os.path.join(tmp, "no.bin"), os.path.join(tmp, "no.fa"), os.path.join(tmp, "out"), exe=exe, **env)
        text = [s.replace(tmp, TMP_TOKEN) for s in (r.stdout, r.stderr)]
    return "\t".join([",".join("%s=%s" % kv for kv in env.items()) or "-", str(r.returncode), json.dumps(text[0]), json.dumps(text[1])])
