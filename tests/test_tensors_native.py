"""The C++ dense-cell tests (csrc/tests/tensor_tests.cpp): the host conversions of gol/cells.hpp against a per-cell loop,
all four element types, the three packed layouts, tail words of 1 and 63 cells, and the refusals."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_tensor_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_tensor_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
