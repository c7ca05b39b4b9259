"""Runs the C++ Larger than Life test binary (host-only: the rule strings with every rejection, the folding of the
middle flag into thresholds with its clamps, and cpu::superstep under seven rules, both boundaries, against a per-cell
count)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_ltl_unit():
    r = subprocess.run([os.path.join(REPO, "build", "gol_ltl_unit")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
