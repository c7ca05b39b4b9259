"""Connected components on the HIP backend: the k_cc_* kernels through components(), count_components(),
components_tensor() and SoupBatch.components() / component_counts(), exact against the numpy oracle
``ops.numpy_components`` on ``sim.board()`` and ``batch.boards()`` (components_cases.py holds the cases; test_components.py
runs them on the CPU backend).  Besides the shared boards: 64 x 4160 (65 words: a second lane group of one lane) and
300 x 64 (the row stride)."""
import numpy as np
import pytest

import components_cases as cc

pytestmark = pytest.mark.gpu

BACKEND = "hip"
BOARDS = cc.BOARDS + cc.HIP_BOARDS


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=cc.bid)
def test_placed_objects(gol, shape, boundary):
    cc.check_placed(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=cc.bid)
def test_random_boards(gol, shape, boundary):
    cc.check_random(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=cc.bid)
def test_components_tensor(gol, shape, boundary):
    cc.check_tensor(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", BOARDS, ids=cc.bid)
def test_adversarial_boards(gol, shape, boundary):
    cc.check_adversarial(gol, BACKEND, shape, boundary)


def test_current_board(gol):
    cc.check_current_board(gol, BACKEND)


def test_truncation(gol):
    cc.check_truncation(gol, BACKEND)


def test_refusals(gol):
    cc.check_refusals(gol, BACKEND, pytest)


def test_two_ranks_refused(gol):
    cc.check_two_ranks(gol, BACKEND)


@pytest.mark.parametrize("size", [64, 128, 256])
def test_soups(gol, size):
    """The HIP records equal the oracle's on the HIP batch's own boards, and equal the CPU backend's."""
    hip = cc.check_soups(gol, BACKEND, size)
    boards = cc.soup_boards(size)
    cpu = gol.SoupBatch.from_boards(boards, backend="cpu").components("moore")
    for a, b in zip(hip["moore"], cpu):
        assert np.array_equal(a, b)
