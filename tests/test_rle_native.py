"""Runs the C++ RLE test binary (host-only: reader and writer round trips on random patterns, counted '$', short
and missing rows, every rejection with the character or offset it names, the 70-column lines, S/B rule headers)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_rle_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_rle_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
