"""The C++ signature tests (csrc/tests/signature_tests.cpp): cpu::superstep's per-generation signatures of a tile's own
cells and cpu::signature against a byte-per-cell loop that applies the definition per cell, on both boundaries."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_signature_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_signature_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
