"""CPU test (no GPU) of the command-line tool's whole route matrix: every combination of LCB_TABLES, LCB_JUNCTIONS, LCB_HANDOVER, LCB_LOAD
and LCB_GPUS at unset, their values and an unknown one, LCB_SEEDS=x alone and beside each other switch, and every switch alone and empty
(tests/cli_inputs.route_matrix) ends with the exit status, stdout and stderr that tests/golden/cli_routes.tsv records from the tool as it
was before its refusals became one ordered list. That pins which of two faults in one command line is reported, for all of them. The
inputs do not exist, so every run ends before any GPU work."""
from concurrent.futures import ThreadPoolExecutor

from tests import cli_inputs


def test_every_setting_of_the_route_switches_answers_as_recorded(built):
    with open(cli_inputs.ROUTES_TSV) as f:
        want = f.read().splitlines()
    runs = cli_inputs.route_matrix()
    assert len(runs) == len(want) == 228
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(cli_inputs.route_run, runs))
    gpu = cli_inputs.has_gpu()
    for g, w in zip(got, want):
        if gpu and w.split("\t")[3].startswith('"error: no HIP device'):      # (only lcb_graph_build looks for the device before the files)
            g, w = g.split("\t")[:3], w.split("\t")[:3]
        assert g == w
