"""The C++ density-film tests (csrc/tests/density_film_tests.cpp): the CPU stepper's per-generation density maps, summed
over 1 to 4 thread ranks, against a byte-per-cell loop, for random rules on every neighbourhood and both boundaries; and
the parsing of GOL_DENSITY_FILM."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_density_film_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_density_film_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
