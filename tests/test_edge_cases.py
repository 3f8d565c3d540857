"""Edge cases (empty seed list, identical genomes, tiny records, several FASTA files, IUPAC / lower case, everything filtered by
the abundance threshold, small b / large m, k = 25 with repeats).
CPU: the C oracle must write what the real reference binary wrote for the same input (stored under tests/golden/edge_cases by
tests/golden/make_edge_cases.py; where oracle/_ref exists the reference is run again and must still write it). GPU: the product CLI
must agree with the reference, live and stored."""
import os
import re

import pytest

from tests import edge_inputs as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "edge_cases")


def _summary(stdout):
    return re.findall(r"^(Blocks found: .*|Coverage: .*)$", stdout, re.M)


def _golden(name, fn):
    with open(os.path.join(GOLDEN, name, fn)) as f:
        return f.read()


@pytest.mark.parametrize("name", E.NAMES)
def test_oracle_agrees_with_reference_on_edge_cases(built, name, tmp_path):
    case = E.build(name, str(tmp_path))
    b = E.run_cli(os.path.join(ROOT, "oracle", "lcb_oracle"), case, str(tmp_path / "orc"))
    assert b.returncode == 0, b.stderr
    assert open(str(tmp_path / "orc" / "blocks_coords.gff")).read() == _golden(name, "blocks_coords.gff")
    assert _summary(b.stdout) == _golden(name, "summary.txt").splitlines()
    ref = os.path.join(ROOT, "oracle", "_ref", "sibeliaz-lcb-ref")
    if os.path.exists(ref):          # (the stored output is still the reference's)
        a = E.run_cli(ref, case, str(tmp_path / "ref"), ["--noseq"])
        assert a.returncode == 0, a.stderr
        assert open(str(tmp_path / "ref" / "blocks_coords.gff")).read() == _golden(name, "blocks_coords.gff")
        assert _summary(a.stdout) == _golden(name, "summary.txt").splitlines()


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.NAMES)
def test_cli_matches_reference_on_edge_cases(built, name, tmp_path):
    case = E.build(name, str(tmp_path))
    exe = os.path.join(ROOT, "sibeliaz_amd", "bin", "sibeliaz-lcb")
    a = E.run_cli(E.reference_exe(), case, str(tmp_path / "ref"), ["--noseq"])
    b = E.run_cli(exe, case, str(tmp_path / "gpu"), ["--chunks", "3"])
    assert a.returncode == 0, a.stderr
    assert b.returncode == 0, b.stderr
    assert open(str(tmp_path / "gpu" / "blocks_coords.gff")).read() == open(str(tmp_path / "ref" / "blocks_coords.gff")).read()
    assert _summary(a.stdout) == _summary(b.stdout)
    assert open(str(tmp_path / "gpu" / "blocks_coords.gff")).read() == _golden(name, "blocks_coords.gff")
    assert _summary(b.stdout) == _golden(name, "summary.txt").splitlines()
    for i in range(3):                   # block sequences for the aligner (blocksfinder.h:533-582), as the reference wrote them
        assert open(str(tmp_path / "gpu" / ("%d.tmp" % i))).read() == _golden(name, "seq_%d.txt" % i)
    if os.path.basename(E.reference_exe()) == "sibeliaz-lcb-ref":          # block sequences for the aligner (blocksfinder.h:533-582)
        c = E.run_cli(E.reference_exe(), case, str(tmp_path / "refseq"), ["--chunks", "3"])
        assert c.returncode == 0
        for i in range(3):
            assert open(str(tmp_path / "gpu" / ("%d.tmp" % i))).read() == open(str(tmp_path / "refseq" / ("%d.tmp" % i))).read()
