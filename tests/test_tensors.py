"""The tensor readers and writers on the CPU backend: every method against its numpy twin over dtypes and boards, the
load round trips with the odd values, step_film's record rules, ops.evolve, every refusal, and thread ranks.

The CPU backend runs the Python layer, the bindings and the host conversions of gol/cells.hpp, which share their source
description with the device kernels (test_gpu_tensors.py runs those).  All comparisons are exact (tensor_cases.py)."""
import numpy as np
import pytest
import torch

import tensor_cases as tc
import wide_cases as wc
from gol_amd.ops import numpy_step_rule, random_board


def _sim(gol, shape, **kw):
    kw.setdefault("backend", "cpu")
    return gol.Simulation(shape[0], width=shape[1], **kw)


@pytest.mark.parametrize("shape", tc.BOARDS, ids=tc.bid)
@pytest.mark.parametrize("name", tc.DTYPES)
def test_board_and_window(gol, name, shape):
    """board_tensor() is board(); window_tensor() is window(), for the whole board from the middle (both seams) and
    for its last row and column."""
    H, W = shape
    s = _sim(gol, shape, rule=tc.HIGHLIFE).init(5, seed=tc.SEED)
    s.step(tc.GENS)
    ref = tc.board_after(H, W, tc.SEED, tc.HIGHLIFE, "torus", tc.GENS)
    assert np.array_equal(s.board(), ref)
    t = s.board_tensor(dtype=tc.dt(name))
    assert not t.is_cuda and tuple(t.shape) == shape
    tc.assert_cells(t, name, ref)
    for rect in [(H // 3, W // 2 + 1, H, W), (H - 1, 0, 1, W), (0, W - 1, H, 1)]:
        w = s.window_tensor(*rect, dtype=tc.dt(name))
        twin = s.window(*rect)
        assert np.array_equal(twin, tc.torus_window(ref, *rect))
        tc.assert_cells(w, name, twin)
    out = torch.empty(shape, dtype=tc.dt(name))
    assert s.board_tensor(out=out) is out
    tc.assert_cells(out, name, ref)
    assert s.board_tensor().dtype == torch.uint8  # the default


@pytest.mark.parametrize("shape", tc.BOARDS, ids=tc.bid)
@pytest.mark.parametrize("name", tc.DTYPES)
def test_envelope(gol, name, shape):
    H, W = shape
    s = _sim(gol, shape, rule=tc.HIGHLIFE, envelope=True).init(5, seed=tc.SEED)
    s.step(tc.GENS)
    start, e = s.envelope_tensor(dtype=tc.dt(name))
    twin_start, twin = s.envelope()
    assert start == twin_start == 0
    assert np.array_equal(twin, tc.envelope_of(H, W, tc.SEED, tc.HIGHLIFE, tc.GENS))
    tc.assert_cells(e, name, twin)


@pytest.mark.parametrize("shape", tc.BOARDS, ids=tc.bid)
@pytest.mark.parametrize("name", tc.DTYPES)
def test_step_film(gol, name, shape):
    """step_film() is numpy_film for the whole board from the middle (across both seams), and the board follows."""
    H, W = shape
    rect = (H // 3, W // 2 + 1, H, W)
    gens = 5
    s = _sim(gol, shape, rule=tc.HIGHLIFE, film=rect).init(5, seed=tc.SEED)
    f = s.step_film(gens, dtype=tc.dt(name))
    assert tuple(f.shape) == (gens, H, W)
    tc.assert_cells(f, name, tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, "torus", gens, rect))
    assert s.generation == gens
    assert np.array_equal(s.board(), tc.board_after(H, W, tc.SEED, tc.HIGHLIFE, "torus", gens))


@pytest.mark.parametrize("shape", tc.BOARDS, ids=tc.bid)
@pytest.mark.parametrize("name", tc.DTYPES)
def test_load_round_trip(gol, name, shape):
    """load_tensor() of the odd values (2, -1, 0.5 and NaN alive, -0.0 dead) is set_board() of their != 0; the board
    steps on from it, and board_tensor() gives it back."""
    H, W = shape
    t, alive = tc.odd_cells(shape, name, seed=H * 1000 + W)
    s = _sim(gol, shape, rule=tc.HIGHLIFE).init(5, seed=1)
    assert s.load_tensor(t) is s
    assert np.array_equal(s.board(), alive)
    tc.assert_cells(s.board_tensor(dtype=tc.dt(name)), name, alive)
    s.step(9)
    assert np.array_equal(s.board(), numpy_step_rule(alive, tc.HIGHLIFE, 9))


def test_load_values_by_hand(gol):
    s = _sim(gol, (1, 7)).init(0)
    for name in tc.FLOATS:
        s.load_tensor(torch.tensor([[0.0, -0.0, float("nan"), 2.0, -1.0, 0.5, 1.0]], dtype=tc.dt(name)))
        assert s.board().tolist() == [[0, 0, 1, 1, 1, 1, 1]], name
    s.load_tensor(torch.tensor([[0, 1, 2, 255, 0, 128, 0]], dtype=torch.uint8))
    assert s.board().tolist() == [[0, 1, 1, 1, 0, 1, 0]]
    # a non-contiguous input is taken (made contiguous); it resets the envelope as set_board() does
    e = _sim(gol, (64, 64), envelope=True).init(5, seed=2)
    e.step(4)
    cells = torch.from_numpy(random_board(64, 64, 8).copy())
    e.load_tensor(cells.t())
    assert np.array_equal(e.board(), cells.numpy().T)
    start, env = e.envelope_tensor()
    assert start == 4 and np.array_equal(env.numpy(), cells.numpy().T)


def test_step_film_record_rules(gol):
    H, W, rect = 65, 65, (60, 60, 10, 10)
    s = _sim(gol, (H, W), rule=tc.HIGHLIFE, film=rect).init(5, seed=tc.SEED)
    s.step(2)
    with pytest.raises(ValueError, match=r"2 frames.*film_clear\(\)"):  # a non-empty record is refused
        s.step_film(3)
    assert s.generation == 2 and s.film()[1].shape[0] == 2  # (nothing ran, the record is whole)
    s.film_clear()
    f = s.step_film(4)
    tc.assert_cells(f, "uint8", tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, "torus", 6, rect)[2:])
    start, frames = s.film()
    assert start == 6 == s.generation and frames.shape == (0, 10, 10)  # empty, and it starts where the board stands
    s.step(3)
    start, frames = s.film()
    assert start == 6 and np.array_equal(frames, tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, "torus", 9, rect)[6:])
    s.film_clear()
    empty = s.step_film(0)
    assert tuple(empty.shape) == (0, 10, 10) and s.generation == 9
    # a second call right after the first: the record it left is empty
    g = s.step_film(2, dtype=torch.float32)
    tc.assert_cells(g, "float32", tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, "torus", 11, rect)[9:])


@pytest.mark.parametrize("size", [64, 128, 256])
@pytest.mark.parametrize("name", tc.DTYPES)
def test_soups(gol, name, size):
    """boards_tensor() is boards(), for all soups and for a range in the middle; from_tensor() starts the same batch."""
    b = gol.SoupBatch(9, size, rule=tc.HIGHLIFE, backend="cpu", seed=5)
    b.step(3)
    tc.assert_cells(b.boards_tensor(dtype=tc.dt(name)), name, b.boards())
    tc.assert_cells(b.boards_tensor(range(2, 6), dtype=tc.dt(name)), name, b.boards(range(2, 6)))
    tc.assert_cells(b.boards_tensor([7], dtype=tc.dt(name)), name, b.boards([7]))
    t, alive = tc.odd_cells((4, size, size), name, seed=size)
    c = gol.SoupBatch.from_tensor(t, rule=tc.HIGHLIFE)
    assert c.backend == "cpu" and c.n == 4 and c.size == size
    assert np.array_equal(c.boards(), alive)
    c.step(5)
    ref = np.stack([numpy_step_rule(a, tc.HIGHLIFE, 5) for a in alive])
    tc.assert_cells(c.boards_tensor(dtype=tc.dt(name)), name, ref)
    res = gol.SoupBatch.from_tensor(t[:2], rule=tc.HIGHLIFE).settle(64)  # the search runs on a batch from a tensor
    assert res.period.shape == (2,)


@pytest.mark.parametrize("name", tc.DTYPES)
def test_evolve(gol, name):
    for shape, rule, gens in [((64, 64), "B3/S23", 7), ((3, 128, 128), tc.HIGHLIFE, 5), ((2, 256, 256), "B3/S23", 2)]:
        x, alive = tc.odd_cells(shape, name, seed=sum(shape))
        y = gol.ops.evolve(x, gens, rule=rule)
        assert y.shape == x.shape and y.dtype == x.dtype and y.device == x.device and y is not x
        boards = alive.reshape((-1,) + shape[-2:])
        ref = np.stack([numpy_step_rule(b, rule, gens) for b in boards]).reshape(shape)
        tc.assert_cells(y, name, ref)
    x = torch.zeros((64, 64), dtype=tc.dt(name))
    tc.assert_cells(gol.ops.evolve(x, 0), name, np.zeros((64, 64), np.uint8))


def test_value_errors(gol):
    s = _sim(gol, (65, 70)).init(5, seed=3)
    before = s.board()
    bad = [
        (lambda: s.board_tensor(dtype=torch.int32), "torch.int32"),
        (lambda: s.board_tensor(dtype=torch.float64), "torch.float64"),
        (lambda: s.board_tensor(out=torch.empty((65, 71), dtype=torch.uint8)), r"\(65, 71\)"),
        (lambda: s.board_tensor(out=torch.empty((70, 65), dtype=torch.uint8).t()), "not contiguous"),
        (lambda: s.board_tensor(out=torch.empty((65, 140), dtype=torch.uint8)[:, ::2]), "not contiguous"),
        (lambda: s.board_tensor(dtype=torch.float16, out=torch.empty((65, 70), dtype=torch.uint8)), "torch.uint8"),
        (lambda: s.board_tensor(out=np.zeros((65, 70), np.uint8)), "ndarray"),
        (lambda: s.load_tensor(torch.zeros((65, 71))), r"\(65, 71\)"),
        (lambda: s.load_tensor(torch.zeros((65, 70), dtype=torch.int64)), "torch.int64"),
        (lambda: s.load_tensor(np.zeros((65, 70), np.uint8)), "ndarray"),
        (lambda: s.window_tensor(0, 0, 66, 3), "66 x 3"),
        (lambda: s.window_tensor(0, 0, 3, 0), "3 x 0"),
        (lambda: s.window_tensor(0, 0, 3, 3, out=torch.empty((3, 4), dtype=torch.uint8)), r"\(3, 4\)"),
        (lambda: s.envelope_tensor(), "envelope=True"),
        (lambda: s.step_film(3), "film="),
    ]
    for call, what in bad:
        with pytest.raises(ValueError, match=what):
            call()
    assert np.array_equal(s.board(), before) and s.generation == 0
    d = _sim(gol, (65, 70), boundary="dead").init(5, seed=3)
    with pytest.raises(ValueError, match="does not lie inside"):
        d.window_tensor(60, 60, 10, 5)
    f = _sim(gol, (65, 70), film=(0, 0, 4, 4)).init(5, seed=3)
    with pytest.raises(ValueError, match="negative"):
        f.step_film(-1)
    with pytest.raises(ValueError, match=r"\(2, 4, 4\)"):
        f.step_film(3, out=torch.empty((2, 4, 4), dtype=torch.uint8))
    assert f.generation == 0
    b = gol.SoupBatch(6, 64, backend="cpu")
    for idx, what in [([0, 2], "no contiguous range"), (range(0, 6, 2), "no contiguous range"), ([3, 2], "no contiguous range"),
                      ([], "empty"), (range(4, 8), "outside 0 .. 5"), ([-1, 0], "outside 0 .. 5")]:
        with pytest.raises(ValueError, match=what):
            b.boards_tensor(idx)
    with pytest.raises(ValueError, match=r"\(6, 64, 64\)"):
        b.boards_tensor(out=torch.empty((5, 64, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="torch.int16"):
        b.boards_tensor(dtype=torch.int16)
    with pytest.raises(ValueError, match=r"\(2, 64, 65\)"):
        gol.SoupBatch.from_tensor(torch.zeros((2, 64, 65)))
    with pytest.raises(ValueError, match="size 96"):
        gol.SoupBatch.from_tensor(torch.zeros((2, 96, 96)))
    with pytest.raises(ValueError, match="backend 'hip'"):
        gol.SoupBatch.from_tensor(torch.zeros((2, 64, 64)), backend="hip")
    for shape in [(96, 96), (2, 64, 128), (64,), (1, 2, 64, 64), (0, 64, 64)]:
        with pytest.raises(ValueError, match="evolve"):
            gol.ops.evolve(torch.zeros(shape), 1)
    with pytest.raises(ValueError, match="torch.int32"):
        gol.ops.evolve(torch.zeros((64, 64), dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="negative"):
        gol.ops.evolve(torch.zeros((64, 64)), -1)
    with pytest.raises(ValueError):  # a V rule: soup batches run Moore rules
        gol.ops.evolve(torch.zeros((64, 64)), 1, rule="B13/S13V")
    # the native checks stand behind the Python ones: a wrong element count or type code never reaches a conversion
    t = torch.zeros((65, 70), dtype=torch.uint8)
    with pytest.raises(ValueError, match="4549 elements"):
        s.engine.read_tile_cells(t.data_ptr(), 0, t.numel() - 1)
    with pytest.raises(ValueError, match="code 7"):
        s.engine.read_tile_cells(t.data_ptr(), 7, t.numel())
    with pytest.raises(ValueError, match="not aligned"):
        s.engine.read_tile_cells(t.data_ptr() + 1, 3, t.numel())


RANKS = [(3, 96, 200, {}), (4, 128, 256, {"decomp": "2d", "grid": "2x2"})]


@pytest.mark.parametrize("P,H,W,kw", RANKS, ids=["1d3", "2x2"])
def test_thread_ranks(gol, P, H, W, kw):
    """Every rank's board_tensor() is its board(), load_tensor() sets its own tile, and the one-rank calls raise on
    every rank, naming the rank count."""
    rect = (28, 50, 10, 30)

    def script(s):
        s.step(5)
        own = s.board()
        got = {n: tc.exact01(s.board_tensor(dtype=tc.dt(n)), n) for n in tc.DTYPES}
        refused = []
        for call in (lambda: s.window_tensor(0, 0, 4, 4), lambda: s.step_film(2)):
            try:
                call()
                refused.append(None)
            except ValueError as e:
                refused.append(str(e))
        s.load_tensor(torch.from_numpy(1 - own))
        flipped = s.board()
        s.load_tensor(torch.from_numpy(own.copy()).to(torch.float32))
        return own, got, refused, flipped, s.generation

    parts = wc.run_ranks(gol, P, H, W, "cpu", script, rule=tc.HIGHLIFE, film=rect, **kw)
    ref = wc.assemble(H, W, parts)
    assert np.array_equal(ref, numpy_step_rule(random_board(H, W, wc.SEED), tc.HIGHLIFE, 5))
    for p in parts:
        own, got, refused, flipped, gen = p.result
        for n in tc.DTYPES:
            assert np.array_equal(got[n], own), (p.rank, n)
        assert all(r is not None and f"{P} ranks" in r for r in refused), refused
        assert np.array_equal(flipped, 1 - own) and np.array_equal(p.board, own) and gen == 5
