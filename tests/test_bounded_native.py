"""Runs the C++ bounded-board test binary (host-only: cpu::superstep with dead edges against a byte-per-cell loop
for tiles at every position of a 3 x 3 rank grid, unaligned widths and every depth up to the halo, the one-rank
case through the torus ghost fills, and the RLE topology suffix parser with every rejection)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_bounded_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_bounded_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
