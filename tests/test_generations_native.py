"""Runs the C++ Generations test binary (host-only: the B/S/C rule strings with every rejection and the code()
round trip, and cpu::superstep on planes with cpu::state_counts under six rules, both boundaries, against a
byte-per-cell loop of states)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_generations_unit():
    r = subprocess.run([os.path.join(REPO, "build", "gol_generations_unit")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
