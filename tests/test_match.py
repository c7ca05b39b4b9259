"""Pattern matching on the CPU backend: match(), count_matches(), match_tensor() and SoupBatch.match_counts() against the
numpy oracle ``ops.numpy_match`` (match_cases.py holds the cases; test_gpu_match.py runs them on the HIP backend), and the
oracle and the templates themselves on hand-made boards."""
import numpy as np
import pytest

import match_cases as mc
from gol_amd.ops import match_template, numpy_match, template_orientations

BACKEND = "cpu"


def test_oracle_by_hand():
    """numpy_match on boards small enough to read: positions, both boundaries, the ring, orientation ids."""
    b = np.zeros((8, 8), dtype=np.uint8)
    b[0, 0] = b[0, 7] = b[7, 0] = b[7, 7] = 1  # a block on the torus corner
    block = match_template(mc.BLOCK)
    pos, ids = numpy_match(b, block, "torus")
    assert pos.tolist() == [[7, 7]] and ids.tolist() == [0]
    assert len(numpy_match(b, block, "dead")[0]) == 0
    b2 = np.zeros((8, 8), dtype=np.uint8)
    b2[0:2, 0:2] = 1  # flush in the corner of a bounded board: the ring lies off the board
    assert numpy_match(b2, block, "dead")[0].tolist() == [[0, 0]]
    b2[0, 3] = 1  # a cell just outside the ring
    assert numpy_match(b2, block, "dead")[0].tolist() == [[0, 0]]
    b2[1, 2] = 1  # a cell inside the ring
    assert len(numpy_match(b2, block, "dead")[0]) == 0
    assert numpy_match(b2, match_template(mc.BLOCK, 0), "dead")[0].tolist() == [[0, 0]]
    # a vertical blinker is orientation 1 of the horizontal one, reported at its top cell
    b3 = np.zeros((8, 8), dtype=np.uint8)
    b3[2:5, 4] = 1
    pos, ids = numpy_match(b3, match_template(mc.BLINKER), "torus", "all")
    assert pos.tolist() == [[2, 4]] and ids.tolist() == [1]
    assert len(numpy_match(b3, match_template(mc.BLINKER), "torus")[0]) == 0


def test_templates():
    t = match_template(mc.GLIDER)
    assert t.shape == (5, 5) and t.ring == 1 and t.care.all()
    assert np.array_equal(t.value[1:4, 1:4], mc.GLIDER_CELLS) and t.value.sum() == 5
    assert t == match_template(mc.GLIDER_CELLS, margin=1) and t != match_template(mc.GLIDER_CELLS, margin=0)
    with pytest.raises(AttributeError):
        t.ring = 2
    with pytest.raises(ValueError):
        t.value[0, 0] = 1
    for pattern, n in ((mc.BLOCK, 1), (mc.BLINKER, 2), (mc.BEEHIVE, 2), (mc.GLIDER_CELLS, 8)):
        t = match_template(pattern)
        mine = template_orientations(t)
        native = t.native.orientations(True)
        assert len(mine) == len(native) == n
        for (k, o), (kn, on) in zip(mine, native):  # the numpy orientations are the native ones, id by id
            assert k == kn and o.ring == on.ring
            assert np.array_equal(o.value, on.value) and np.array_equal(o.care, on.care)
            assert np.array_equal(o.value, np.pad(mc.turned(np.asarray(pattern), k), 1))
    assert [k for k, _ in template_orientations(match_template(mc.BLINKER), False)] == [0]


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", mc.BOARDS, ids=mc.bid)
def test_placed_gliders(gol, shape, boundary):
    mc.check_placed_gliders(gol, BACKEND, shape, boundary)
    mc.check_eight_orientations(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", mc.BOARDS, ids=mc.bid)
def test_random_boards(gol, shape, boundary):
    mc.check_random(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", mc.BOARDS, ids=mc.bid)
def test_current_board(gol, shape, boundary):
    mc.check_current_board(gol, BACKEND, shape, boundary)


def test_truncation(gol):
    mc.check_truncation(gol, BACKEND)


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
@pytest.mark.parametrize("shape", mc.BOARDS, ids=mc.bid)
def test_match_tensor(gol, shape, boundary):
    mc.check_tensor(gol, BACKEND, shape, boundary)


def test_refusals(gol):
    mc.check_refusals(gol, BACKEND, pytest)


def test_two_ranks_refused(gol):
    mc.check_two_ranks(gol, BACKEND)


def test_placed_soups(gol):
    mc.check_placed_soups(gol, BACKEND)


def test_random_soups(gol):
    mc.check_random_soups(gol, BACKEND)
