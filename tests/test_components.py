"""Connected components on the CPU backend: components(), count_components(), components_tensor() and
SoupBatch.components() / component_counts() against the numpy oracle ``ops.numpy_components`` (components_cases.py holds the
cases; test_gpu_components.py runs them on the HIP backend), and the oracle and the hash themselves: by hand, against
scipy.ndimage.label, and on a list of small objects whose hashes must differ."""
import time

import numpy as np
import pytest

import components_cases as cc
from gol_amd.ops import numpy_components, object_hash, random_board

BACKEND = "cpu"


def test_oracle_by_hand():
    """numpy_components on boards small enough to read: labels, anchors, the box rule on both boundaries, the hash."""
    b = np.zeros((8, 10), dtype=np.uint8)
    b[0, 0] = b[0, 9] = b[7, 0] = b[7, 9] = 1  # a block on the torus corner
    b[3, 4] = b[4, 5] = 1                      # a diagonal pair
    labels, res = numpy_components(b, "moore", "torus")
    assert res.count == 2 and res.anchor.tolist() == [[0, 0], [3, 4]] and res.population.tolist() == [4, 2]
    assert res.bbox.tolist() == [[7, 9, 2, 2], [3, 4, 2, 2]]
    assert labels[0, 0] == labels[7, 9] == 1 and labels[3, 4] == labels[4, 5] == 1 + 3 * 10 + 4 and labels[1, 1] == 0
    assert int(res.hash[0]) == object_hash(cc.BLOCK) and int(res.hash[1]) == object_hash(np.eye(2, dtype=np.uint8))
    _, dead = numpy_components(b, "moore", "dead")
    assert dead.count == 5 and dead.bbox[0].tolist() == [0, 0, 1, 1]
    _, vn = numpy_components(b, "von_neumann", "torus")
    assert vn.count == 3  # the diagonal pair falls apart
    far = np.zeros((8, 10), dtype=np.uint8)
    far[2, 2] = far[2, 4] = far[6, 2] = far[6, 5] = 1
    assert numpy_components(far, "moore", "torus")[1].count == 4 and numpy_components(far, "moore2", "torus")[1].count == 3
    # more than half of an axis: the smaller of the two frames; the whole axis: the plain frame
    row = np.zeros((8, 10), dtype=np.uint8)
    row[2, [8, 9, 0, 1, 2, 3]] = 1
    assert numpy_components(row, "moore", "torus")[1].bbox.tolist() == [[2, 8, 1, 6]]
    row[2, :] = 1
    assert numpy_components(row, "moore", "torus")[1].bbox.tolist() == [[2, 0, 1, 10]]
    with pytest.raises(ValueError, match="hex"):
        numpy_components(b, "hex")
    with pytest.raises(ValueError, match="not 0 or 1"):
        numpy_components(b * 2)


def test_hash_orientations_and_distinctness():
    """The hash is one for the eight orientations and wherever the object lies; block, blinker, beehive, both glider
    phases, boat, tub, loaf, ship, pond, a single cell, domino, L-tromino and I-tetromino have 14 distinct hashes."""
    for cells in cc.DISTINCT:
        assert len({object_hash(cc.turned(cells, k)) for k in range(8)}) == 1
        assert object_hash(np.pad(cells, ((3, 0), (1, 5)))) == object_hash(cells)
        from gol_amd import native

        assert native.object_hash(cells) == object_hash(cells)  # the native formula (per-cell keys) and np.rot90 agree
    assert len({object_hash(c) for c in cc.DISTINCT}) == len(cc.DISTINCT) == 14


@pytest.mark.parametrize("nb,structure", [("von_neumann", [[0, 1, 0], [1, 1, 1], [0, 1, 0]]), ("moore", np.ones((3, 3), int))])
def test_oracle_against_scipy(nb, structure):
    """The oracle's partition equals scipy.ndimage.label's on bounded boards (this guards the oracle itself)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    for shape in ((70, 130), (64, 64)):
        for density in cc.DENSITIES:
            board = cc.random_cells(shape, density)
            labels, res = numpy_components(board, nb, "dead")
            theirs, n = ndimage.label(board, structure=structure)
            assert n == res.count
            # the same partition: every cell's label is 1 + the first cell of its scipy object
            flat = theirs.ravel()
            idx = np.flatnonzero(flat)
            firsts = np.full(n + 1, flat.size, dtype=np.int64)
            np.minimum.at(firsts, flat[idx], idx)
            assert np.array_equal(labels.ravel()[idx], 1 + firsts[flat[idx]])
            assert not labels.ravel()[flat == 0].any()


def test_oracle_is_vectorised():
    """64 x 4160 at density 0.5 under 0.2 s (best of three): hooking and compression over edge lists, no per-cell loop."""
    board = random_board(64, 4160, cc.mc.SEED)
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        numpy_components(board, "moore", "torus")
        best = min(best, time.perf_counter() - t0)
    assert best < 0.2, best


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", cc.BOARDS, ids=cc.bid)
def test_placed_objects(gol, shape, boundary):
    cc.check_placed(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", cc.BOARDS, ids=cc.bid)
def test_random_boards(gol, shape, boundary):
    cc.check_random(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", cc.BOARDS, ids=cc.bid)
def test_components_tensor(gol, shape, boundary):
    cc.check_tensor(gol, BACKEND, shape, boundary)


@pytest.mark.parametrize("boundary", cc.BOUNDARIES)
@pytest.mark.parametrize("shape", cc.BOARDS, ids=cc.bid)
def test_adversarial_boards(gol, shape, boundary):
    cc.check_adversarial(gol, BACKEND, shape, boundary)


def test_checkerboard_64x4160(gol):
    """133120 one-cell objects under von Neumann, below the default max_objects; one component under Moore."""
    board = cc.adversarial((64, 4160))["checkerboard"]
    s = gol.Simulation(64, width=4160, backend=BACKEND).init(0)
    s.set_board(board)
    res = s.components("von_neumann")
    assert res.count == 64 * 4160 // 2 == 133120 and not res.truncated and len(set(res.hash.tolist())) == 1
    assert s.count_components("moore") == 1


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
    cc.check_soups(gol, BACKEND, size)
