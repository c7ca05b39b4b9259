"""The C++ film tests (csrc/tests/film_tests.cpp): cpu::superstep's per-generation packed frames of a board window
against a byte-per-cell loop, on 3 x 3 rank grids, unaligned widths, every depth up to the halo, random rules, both
boundaries and noise in the ghost cells; and FilmGeo's word count."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_film_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_film_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
