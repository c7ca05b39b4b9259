"""Pattern matching on the HIP backend: the k_match and k_match_positions kernels through match(), count_matches(),
match_tensor() and SoupBatch.match_counts(), exact against the numpy oracle ``ops.numpy_match`` on ``sim.board()`` and
``batch.boards()`` (match_cases.py holds the cases; test_match.py runs them on the CPU backend).  Besides the shared
boards: 64 x 4160 (65 words: a second lane group of one lane) and 300 x 64 (the row stride)."""
import numpy as np
import pytest

import match_cases as mc

pytestmark = pytest.mark.gpu

BACKEND = "hip"
BOARDS = mc.BOARDS + mc.HIP_BOARDS


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=mc.bid)
def test_placed_gliders(gol, shape, boundary):
    mc.check_placed_gliders(gol, BACKEND, shape, boundary)
    mc.check_eight_orientations(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=mc.bid)
def test_random_boards(gol, shape, boundary):
    mc.check_random(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=mc.bid)
def test_current_board(gol, shape, boundary):
    mc.check_current_board(gol, BACKEND, shape, boundary)


def test_truncation(gol):
    mc.check_truncation(gol, BACKEND)


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=mc.bid)
def test_match_tensor(gol, shape, boundary):
    mc.check_tensor(gol, BACKEND, shape, boundary)


def test_refusals(gol):
    mc.check_refusals(gol, BACKEND, pytest)


def test_two_ranks_refused(gol):
    mc.check_two_ranks(gol, BACKEND)


def test_placed_soups(gol):
    mc.check_placed_soups(gol, BACKEND)


def test_random_soups(gol):
    """The HIP counts equal the oracle's on the HIP batch's own boards, and equal the CPU backend's."""
    mc.check_random_soups(gol, BACKEND)
    for (got, boards, period), (cpu, cpu_boards, cpu_period) in zip(mc.random_soup_counts(gol, BACKEND),
                                                                    mc.random_soup_counts(gol, "cpu")):
        assert np.array_equal(boards, cpu_boards) and np.array_equal(period, cpu_period)
        assert np.array_equal(got, cpu)
