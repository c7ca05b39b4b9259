"""The C++ connected-components tests (csrc/tests/components_tests.cpp): the host labeller of gol/components.hpp against a
byte-per-cell flood fill on random and adversarial boards, both boundaries and all three neighbourhoods; the box rule;
the hash under the eight turns; batches, truncation and the refusals."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gol_components_unit(tmp_path):
    r = subprocess.run([os.path.join(REPO, "build", "gol_components_unit")], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
