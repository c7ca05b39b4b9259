"""Soup batches on the HIP backend: the kernel step_soups (soup_kernel.hip), one wave64 per soup, against the numpy
oracle and the CPU backend.

The cases are soup_cases.py's, shared with test_soups.py (the oracle results are computed once for both files): plain
stepping bit for bit at 64^2, 128^2 and 256^2 (the lane wrap 63 -> 0, the word-half seam, the word seams, the in-lane
rows), seam patterns from arrays, random soups that settle, soups that do not, chunks and resumption; and, here only,
more soups than the card holds at once, waves of one launch that end at different generations, and the CLI on HIP.
Every comparison is exact."""
import numpy as np
import pytest

import soup_cases as sc
from gol_amd.ops import numpy_step_rule
from test_cli import run

pytestmark = pytest.mark.gpu

BACKEND = "hip"


@pytest.mark.parametrize("rule", sc.STEP_RULES)
@pytest.mark.parametrize("S", [64, 128])
def test_plain_steps(gol, S, rule):
    sc.check_plain_steps(gol, BACKEND, S, rule)


@pytest.mark.parametrize("rule", ["B3/S23", "B36/S23"])
def test_plain_steps_256(gol, rule):
    sc.check_plain_steps(gol, BACKEND, 256, rule)


@pytest.mark.parametrize("S", [64, 128])
def test_seam_patterns(gol, S):
    sc.check_patterns(gol, BACKEND, S)


@pytest.mark.parametrize("S,rule,n", sc.SETTLING)
def test_random_soups_settle(gol, S, rule, n):
    sc.check_settling(gol, BACKEND, S, rule, n)


def test_soups_that_do_not_settle(gol):
    sc.check_unsettled(gol, BACKEND)


@pytest.mark.parametrize("S,rule,n", sc.SETTLING[:2])
def test_chunk_independence_and_resumption(gol, S, rule, n):
    sc.check_chunks(gol, BACKEND, S, rule, n)


@pytest.mark.parametrize("workgroup", [64, 128, 256])
def test_more_soups_than_the_card_holds(gol, workgroup):
    """2500 waves: more than the card's wave slots at 256 threads per workgroup, a last workgroup with spare waves."""
    n, gens = 2500, 64
    hip = gol.SoupBatch(n, 64, backend=BACKEND, seed=sc.SEED, workgroup=workgroup)
    cpu = gol.SoupBatch(n, 64, backend="cpu", seed=sc.SEED)
    got, want = hip.settle(gens), cpu.settle(gens)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    idx = [0, 1, 255, 256, 1023, 1024, 2499]
    boards = hip.boards(idx)
    for k, i in enumerate(idx):
        assert np.array_equal(boards[k], numpy_step_rule(sc.soup(64, sc.SEED + i), "B3/S23", int(got.generation[i]))), i
    assert hip.stats()["workgroup"] == workgroup


@pytest.mark.parametrize("n", [1, 3])
def test_few_soups(gol, n):
    hip = gol.SoupBatch(n, 64, backend=BACKEND, seed=sc.SEED)
    res = hip.settle(64)
    assert list(res.generation) == [64] * n
    for i in range(n):
        assert np.array_equal(hip.boards([i])[0], numpy_step_rule(sc.soup(64, sc.SEED + i), "B3/S23", 64))


def test_mixed_settling_times_in_one_launch(gol):
    sb = sc.check_mixed(gol, BACKEND, chunk=512)
    assert sb.stats()["kernel"] == "soups@64"


def test_settle_256(gol):
    """m = 4: the CPU backend (itself checked against the oracle at 64^2 and 128^2) is the reference at 256^2."""
    hip = gol.SoupBatch(3, 256, "B36/S23", backend=BACKEND, seed=sc.SEED)
    cpu = gol.SoupBatch(3, 256, "B36/S23", backend="cpu", seed=sc.SEED)
    for a, b in zip(hip.settle(1500, transient=True, chunk=200), cpu.settle(1500, transient=True)):
        assert np.array_equal(a, b)
    assert np.array_equal(hip.boards(), cpu.boards())


def test_cli_csv_hip(gol_bin, tmp_path):
    n = 8
    out = tmp_path / "soups.csv"
    r = run(gol_bin, [5, 64, sc.MAX_GENS, 256, 0], tmp_path,
            env={"GOL_BACKEND": "hip", "GOL_SOUPS": str(n), "GOL_SOUPS_TRANSIENT": "1", "GOL_SOUPS_OUT": str(out),
                 "GOL_SEED": str(sc.SEED)})
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(f"soups {n} settled {n} of {n} in ")
    assert out.read_text().splitlines() == sc.csv_lines(sc.settling_oracles(64, "B3/S23", n))
