"""Runs the C++ rule test binary (host-only: rule strings, every rejection, the CPU stepper's generic
bit-sliced path under six rules and the 17 single-bit rules against a byte-per-cell loop)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_rule_unit():
    r = subprocess.run([os.path.join(REPO, "build", "gol_rule_unit")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
