"""Soup batches on the HIP backend: the kernel step_soups (soup_kernel.hip), one wave64 per soup, against the numpy
oracle and the CPU backend.

The cases are soup_cases.py's, shared with test_soups.py (the oracle results are computed once for both files): plain
stepping bit for bit at 64^2, 128^2 and 256^2 (the lane wrap 63 -> 0, the word-half seam, the word seams, the in-lane
rows), seam patterns from arrays at every size, random soups that settle, sparse, placed and tiled boards that settle at
128^2 and 256^2, soups that do not, chunks and resumption, max_gens on the generation of the hit; and, here only, more
soups than the card holds at once, spare waves at every size, waves of one launch that end at different generations, and
the CLI on HIP.  Every comparison is exact.

The 18 instantiations step_soups<M, GENERIC, MODE> and the test that reaches the deciding branch of each (plain: the
boards compared after the launch; settle: a hit, `same_soup` true, `period = g - s` and the counter; transient:
kSoupTransientDone after at least one resumed launch, which the test asserts through the number of launches):

    M  GENERIC  MODE       test
    1  false    PLAIN      test_plain_steps[64-B3/S23]
    1  true     PLAIN      test_plain_steps[64-B36/S23], [64-B3678/S34678]
    2  false    PLAIN      test_plain_steps[128-B3/S23]
    2  true     PLAIN      test_plain_steps[128-B36/S23], [128-B3678/S34678]
    4  false    PLAIN      test_plain_steps_256[B3/S23]
    4  true     PLAIN      test_plain_steps_256[B36/S23]
    1  false    SETTLE     test_three_families_settle[64-B3/S23]    (also test_random_soups_settle, test_seam_patterns[64])
    1  true     SETTLE     test_three_families_settle[64-B36/S23]   (also test_random_soups_settle[64-B36/S23-4])
    2  false    SETTLE     test_three_families_settle[128-B3/S23]   (also test_seam_patterns[128])
    2  true     SETTLE     test_three_families_settle[128-B36/S23]  (also test_family_chunks_and_resumption[128-B36/S23])
    4  false    SETTLE     test_three_families_settle[256-B3/S23]   (also test_seam_patterns[256], the [256-B3/S23] chunks)
    4  true     SETTLE     test_three_families_settle[256-B36/S23]  (also test_spare_waves_at_256, the [256-B36/S23] chunks)
    1  false    TRANSIENT  test_three_families_settle[64-B3/S23]
    1  true     TRANSIENT  test_three_families_settle[64-B36/S23]
    2  false    TRANSIENT  test_three_families_settle[128-B3/S23]
    2  true     TRANSIENT  test_three_families_settle[128-B36/S23]
    4  false    TRANSIENT  test_three_families_settle[256-B3/S23]
    4  true     TRANSIENT  test_three_families_settle[256-B36/S23]
"""
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


@pytest.mark.parametrize("S", sc.SIZES)
def test_seam_patterns(gol, S):
    sc.check_patterns(gol, BACKEND, S)


@pytest.mark.parametrize("rule", sc.FAMILY_RULES)
@pytest.mark.parametrize("S", sc.SIZES)
def test_three_families_settle(gol, S, rule):
    """settle(max_gens, transient=True) in chunks of 200 on a sparse, a placed and two tiled boards: the hit of the search
    and the resumed transient walk of step_soups<S / 64, rule != B3/S23, *>; boards_tensor() of the settled batch."""
    sc.check_variant(gol, BACKEND, S, rule)


@pytest.mark.parametrize("S,rule", sc.FAMILY_CHUNKS)
def test_family_chunks_and_resumption(gol, S, rule):
    sc.check_family_chunks(gol, BACKEND, S, rule)


def test_max_gens_on_the_hit(gol):
    sc.check_max_gens_edges(gol, BACKEND)


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


@pytest.mark.parametrize("workgroup", [64, 128, 256])
def test_spare_waves_at_256(gol, workgroup):
    """5 soups of 256^2 under B36/S23 (step_soups<4, true, *>, about 208 VGPRs: one wave per SIMD): 5 is no multiple of 2
    or 4, so the last workgroup of 128 or 256 threads has spare waves, in settle and in transient mode."""
    boards, oracles, names = sc.family_case(256, "B36/S23", tiles=3)
    assert len(names) == 5
    sb = gol.SoupBatch.from_boards(boards, "B36/S23", backend=BACKEND, workgroup=workgroup)
    res = sb.settle(sc.MAX_GENS, transient=True)
    sc.assert_result(res, sb.boards(), oracles)
    st = sb.stats()
    assert (st["workgroup"], st["settled"], st["kernel"]) == (workgroup, 5, "soups@256:rule")


_cpu_128 = {}


@pytest.mark.parametrize("workgroup", [64, 128, 256])
def test_hundreds_of_soups_at_128(gol, workgroup):
    """301 waves of step_soups<2, true, SETTLE> (a last workgroup with spare waves at 128 and 256 threads) against the CPU
    backend, a handful of them against the oracle."""
    n, gens, rule = 301, 64, "B36/S23"
    hip = gol.SoupBatch(n, 128, rule, backend=BACKEND, seed=sc.SEED, workgroup=workgroup)
    if not _cpu_128:
        _cpu_128["res"] = gol.SoupBatch(n, 128, rule, backend="cpu", seed=sc.SEED).settle(gens)
    got, want = hip.settle(gens), _cpu_128["res"]
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    idx = [0, 1, 2, 3, 4, 255, 256, 299, 300]
    boards = hip.boards(idx)
    for k, i in enumerate(idx):
        assert np.array_equal(boards[k], numpy_step_rule(sc.soup(128, sc.SEED + i), rule, int(got.generation[i]))), i
    assert hip.stats()["workgroup"] == workgroup and hip.stats()["kernel"] == "soups@128:rule"


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


def test_mixed_settling_times_in_one_launch_256(gol):
    sb = sc.check_mixed(gol, BACKEND, chunk=512, S=256)
    assert sb.stats()["kernel"] == "soups@256"


def test_settle_256(gol):
    """m = 4, dense random soups: these do not settle at 256^2 within 1500 generations (test_three_families_settle carries
    the settling); the CPU backend (checked against the oracle at every size by test_soups.py) is the reference."""
    hip = gol.SoupBatch(3, 256, "B36/S23", backend=BACKEND, seed=sc.SEED)
    cpu = gol.SoupBatch(3, 256, "B36/S23", backend="cpu", seed=sc.SEED)
    res = hip.settle(1500, transient=True, chunk=200)
    for a, b in zip(res, cpu.settle(1500, transient=True)):
        assert np.array_equal(a, b)
    assert list(res.period) == [0] * 3 and list(res.generation) == [1500] * 3 and list(res.transient) == [-1] * 3
    assert hip.stats()["settled"] == 0
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
