"""The C++ pattern-matching tests (csrc/tests/match_tests.cpp): the host matcher of gol/match.hpp against a byte-per-cell
loop on random boards and templates, both boundaries; orientation ids and dedup (block 1, blinker 2, glider 8); the
builders and the refusals."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_match_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_match_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
