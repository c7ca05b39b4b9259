"""The C++ soup-batch tests (csrc/tests/soup_tests.cpp): the CPU backend of SoupBatch against a byte-per-cell torus with
the same search, on random rules at S = 64 and S = 128; chunk independence, soups given as words and the refusals."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_soup_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_soup_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
