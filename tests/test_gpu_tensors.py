"""The tensor readers and writers on the HIP backend: the kernels k_cells_from_words<T> and k_words_from_cells<T>
(tensor_kernels.hip) behind board_tensor, window_tensor, step_film, envelope_tensor, load_tensor, the soup batches'
boards_tensor / from_tensor and ops.evolve, against the numpy oracles.

Every comparison is exact (tensor_cases.py: a result is first checked bit for bit to hold only the dtype's 0 and 1).  The
shapes are those where the unpack kernel's 16-byte lines can go wrong: rows shorter than a line, rows whose byte length is
no multiple of 16 (lines that cross rows), tail words of 1, 8, 9 and 63 cells, 63 words per row, several blocks, and an
``out`` that is off 16-byte alignment by 1, 3 and 5 elements inside a sentinel-filled store."""
import numpy as np
import pytest
import torch

import film_cases as fc
import tensor_cases as tc
from gol_amd.ops import numpy_film, numpy_step_rule, random_board

pytestmark = pytest.mark.gpu
DEV = 0
CONWAY = "B3/S23"
# buffer parity after an odd number of generations, R halo rows and the ghost word under three kernels and a bounded board
ENGINES = {
    "temporal": dict(kernel="temporal", rule=CONWAY),
    "tile": dict(kernel="tile", rule=CONWAY),
    "rule": dict(kernel="rule", rule=tc.HIGHLIFE),
    "dead": dict(boundary="dead", rule=tc.HIGHLIFE),
}


def _sim(gol, shape, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", DEV)
    return gol.Simulation(shape[0], width=shape[1], **kw)


def _on_device(t):
    assert t.is_cuda and t.device.index == DEV, t.device


# ----- unpack -----


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("shape", tc.GPU_BOARDS, ids=tc.bid)
def test_board_tensor(gol, shape, engine):
    H, W = shape
    kw = ENGINES[engine]
    boundary = kw.get("boundary", "torus")
    s = _sim(gol, shape, **kw).init(5, seed=tc.SEED)
    s.step(tc.GENS)
    ref = tc.board_after(H, W, tc.SEED, kw["rule"], boundary, tc.GENS)
    assert np.array_equal(s.board(), ref)
    for name in tc.DTYPES:
        t = s.board_tensor(dtype=tc.dt(name))
        _on_device(t)
        tc.assert_cells(t, name, ref)
        out = torch.empty(shape, dtype=tc.dt(name), device=f"cuda:{DEV}")
        got = s.board_tensor(out=out)
        assert got is out and got.data_ptr() == out.data_ptr()
        tc.assert_cells(out, name, ref)
    assert s.board_tensor().dtype == torch.uint8
    assert np.array_equal(s.board(), ref)  # (reading changes nothing)


# ----- guarded out: a misaligned address, rows of 65, 137 and 200 cells -----

GUARD_SHAPES = [(65, 65), (137, 137), (137, 200)]


@pytest.mark.parametrize("offset", [1, 3, 5])
@pytest.mark.parametrize("name", tc.SIZED + ["bool", "bfloat16"])
def test_guarded_board_and_window(gol, name, offset):
    for shape in GUARD_SHAPES:
        H, W = shape
        s = _sim(gol, shape, kernel="rule", rule=tc.HIGHLIFE).init(5, seed=tc.SEED)
        s.step(tc.GENS)
        ref = tc.board_after(H, W, tc.SEED, tc.HIGHLIFE, "torus", tc.GENS)
        store, out = tc.guarded(shape, name, offset, f"cuda:{DEV}")
        assert out.data_ptr() % 16 == (offset * out.element_size()) % 16
        assert s.board_tensor(out=out) is out
        tc.assert_cells(out, name, ref)
        tc.assert_guard(store, shape, offset)
        rect = (H - 7, W - 30, 15, 61)  # across both seams; rows of 61 elements
        store, out = tc.guarded(rect[2:], name, offset, f"cuda:{DEV}")
        s.window_tensor(*rect, out=out)
        tc.assert_cells(out, name, tc.torus_window(ref, *rect))
        tc.assert_guard(store, rect[2:], offset)


@pytest.mark.parametrize("offset", [1, 3, 5])
@pytest.mark.parametrize("name", tc.SIZED)
def test_guarded_film_and_soups(gol, name, offset):
    H, W, rect, gens = 137, 200, (130, 185, 15, 33), 6
    s = _sim(gol, (H, W), rule=tc.HIGHLIFE, film=rect).init(5, seed=tc.SEED)
    shape = (gens,) + rect[2:]
    store, out = tc.guarded(shape, name, offset, f"cuda:{DEV}")
    assert s.step_film(gens, out=out) is out
    tc.assert_cells(out, name, tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, "torus", gens, rect))
    tc.assert_guard(store, shape, offset)
    b = gol.SoupBatch(7, 64, rule=tc.HIGHLIFE, backend="hip", seed=3, device=DEV)
    b.step(2)
    shape = (3, 64, 64)
    store, out = tc.guarded(shape, name, offset, f"cuda:{DEV}")
    b.boards_tensor(range(2, 5), out=out)
    tc.assert_cells(out, name, b.boards(range(2, 5)))
    tc.assert_guard(store, shape, offset)


# ----- window_tensor: the seven window shapes of film_cases.py on 137 x 200 -----


@pytest.mark.parametrize("window", list(fc.WINDOWS))
def test_window_shapes(gol, window):
    rect = fc.WINDOWS[window]
    H, W = fc.SHAPE_H, fc.SHAPE_W
    for boundary in fc.BOUNDARIES:
        if boundary == "dead" and window in fc.WRAPPING:
            continue
        s = _sim(gol, (H, W), rule=tc.HIGHLIFE, boundary=boundary).init(5, seed=fc.SHAPE_SEED)
        s.step(tc.GENS)
        ref = tc.torus_window(tc.board_after(H, W, fc.SHAPE_SEED, tc.HIGHLIFE, boundary, tc.GENS), *rect)
        assert np.array_equal(s.window(*rect), ref)
        for name in tc.DTYPES:
            t = s.window_tensor(*rect, dtype=tc.dt(name))
            _on_device(t)
            assert tuple(t.shape) == rect[2:]
            tc.assert_cells(t, name, ref)


# ----- step_film -----

FILM_WINDOWS = {
    "in_word": (137, 200, (30, 70, 9, 5)),
    "x_seam": (137, 200, (5, 190, 30, 21)),
    "whole_board": (137, 200, (45, 101, 137, 200)),
}


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("window", list(FILM_WINDOWS))
def test_step_film(gol, window, K):
    """step_film() is numpy_film and is what step(n); film() gives on a second simulation, both boundaries."""
    H, W, rect = FILM_WINDOWS[window]
    gens = 2 * K + 3
    for boundary in fc.BOUNDARIES:
        if boundary == "dead":
            rect = (min(rect[0], H - rect[2]), min(rect[1], W - rect[3]), rect[2], rect[3])
        ref = tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, boundary, gens, rect)
        assert len({f.tobytes() for f in ref}) >= 2
        kw = dict(rule=tc.HIGHLIFE, boundary=boundary, halo_depth=K, kernel_depth=K, film=rect)
        s = _sim(gol, (H, W), **kw).init(5, seed=tc.SEED)
        name = tc.DTYPES[(K + len(window)) % len(tc.DTYPES)]
        f = s.step_film(gens, dtype=tc.dt(name))
        _on_device(f)
        assert s.stats()["kernel"].startswith("film@"), s.stats()
        tc.assert_cells(f, name, ref)
        twin = _sim(gol, (H, W), **kw).init(5, seed=tc.SEED)
        twin.step(gens)
        start, frames = twin.film()
        assert start == 0
        tc.assert_cells(f, name, frames)
        assert np.array_equal(s.board(), twin.board())
        # the record rules on the device: empty afterwards, starting at the generation reached; then 3 frames
        start, frames = s.film()
        assert start == gens == s.generation and frames.shape[0] == 0
        s.step(3)
        start, frames = s.film()
        assert start == gens and np.array_equal(frames, tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, boundary, gens + 3, rect)[gens:])
        with pytest.raises(ValueError, match=r"film_clear\(\)"):
            s.step_film(1)


def test_step_film_chunks(gol, monkeypatch):
    """A 1 MiB frame buffer: 137 x 4 words a frame, 239 frames a chunk, so 600 generations take three chunks."""
    monkeypatch.setenv("GOL_FILM_MB", "1")
    H, W, rect, gens = 137, 200, (45, 101, 137, 200), 600
    chunk = (1 << 20) // (137 * 4 * 8)
    assert gens > 2 * chunk
    s = _sim(gol, (H, W), rule=tc.HIGHLIFE, film=rect).init(5, seed=tc.SEED)
    f = s.step_film(gens)
    ref = tc.film_of(H, W, tc.SEED, tc.HIGHLIFE, "torus", gens, rect)
    tc.assert_cells(f, "uint8", ref)
    for edge in (chunk - 1, chunk, 2 * chunk - 1, 2 * chunk):  # the frames on either side of a chunk's end differ
        assert not np.array_equal(ref[edge], ref[edge - 1])
    assert s.generation == gens and s.film()[1].shape[0] == 0


@pytest.mark.parametrize("rule", ["B13/S13V", "B2/S34H"])
def test_step_film_neighbourhoods(gol, rule):
    H, W, rect, gens = 137, 200, (130, 190, 15, 21), 11
    s = _sim(gol, (H, W), rule=rule, film=rect).init(5, seed=tc.SEED)
    f = s.step_film(gens, dtype=torch.float16)
    ref = numpy_film(random_board(H, W, tc.SEED), rule, gens, rect)
    assert len({x.tobytes() for x in ref}) >= 2
    tc.assert_cells(f, "float16", ref)


# ----- load -----


@pytest.mark.parametrize("shape", [(65, 65), (137, 200), (50, 3969)], ids=tc.bid)
@pytest.mark.parametrize("name", tc.DTYPES)
def test_load_tensor(gol, name, shape):
    H, W = shape
    cells, alive = tc.odd_cells(shape, name, seed=H + W)
    s = _sim(gol, shape, rule=tc.HIGHLIFE).init(5, seed=1)
    s.step(tc.GENS)  # (the load goes into the buffer the run left current)
    s.load_tensor(cells.to(f"cuda:{DEV}"))
    assert np.array_equal(s.board(), alive)
    tc.assert_cells(s.board_tensor(dtype=tc.dt(name)), name, alive)
    s.step(9)
    assert np.array_equal(s.board(), numpy_step_rule(alive, tc.HIGHLIFE, 9))


# ----- envelope -----


def test_envelope_tensor(gol):
    N, gens = 137, 7
    s = _sim(gol, (N, N), rule=tc.HIGHLIFE, envelope=True).init(5, seed=tc.SEED)
    s.step(gens)
    ref = tc.envelope_of(N, N, tc.SEED, tc.HIGHLIFE, gens)
    assert ref.sum() > tc.board_after(N, N, tc.SEED, tc.HIGHLIFE, "torus", gens).sum()
    for name in tc.DTYPES:
        start, e = s.envelope_tensor(dtype=tc.dt(name))
        _on_device(e)
        assert start == 0
        tc.assert_cells(e, name, ref)
    tc.assert_cells(s.board_tensor(), "uint8", tc.board_after(N, N, tc.SEED, tc.HIGHLIFE, "torus", gens))
    s.load_tensor(torch.from_numpy(ref.copy()).to(f"cuda:{DEV}"))  # resets the envelope, as set_board() does
    start, e = s.envelope_tensor()
    assert start == gens
    tc.assert_cells(e, "uint8", ref)


# ----- soups -----


@pytest.mark.parametrize("size", [64, 128, 256])
def test_soups(gol, size):
    n, g = 300, 6
    boards = np.stack([random_board(size, size, 1000 + i) for i in range(n)])
    idx = range(140, 160)
    ref = np.stack([numpy_step_rule(boards[i], tc.HIGHLIFE, g) for i in idx])
    for name in tc.DTYPES:
        t = torch.from_numpy(boards).to(f"cuda:{DEV}").to(tc.dt(name))
        b = gol.SoupBatch.from_tensor(t, rule=tc.HIGHLIFE)
        assert b.backend == "hip" and b.n == n and b.size == size and b.stats()["kernel"].startswith(f"soups@{size}")
        b.step(g)
        got = b.boards_tensor(idx, dtype=tc.dt(name))
        _on_device(got)
        tc.assert_cells(got, name, ref)
    assert np.array_equal(b.boards(idx), ref)
    # settle() works on a batch that came from a tensor, and agrees with the same boards given as an array
    few = torch.from_numpy(boards[:24]).to(f"cuda:{DEV}")
    res = gol.SoupBatch.from_tensor(few, rule=CONWAY).settle(3000)
    twin = gol.SoupBatch.from_boards(boards[:24], rule=CONWAY, backend="hip", device=DEV).settle(3000)
    assert np.array_equal(res.period, twin.period) and np.array_equal(res.generation, twin.generation)
    assert np.array_equal(res.population, twin.population)
    if size == 64:
        assert (res.period > 0).any()  # (some 64 x 64 soups have settled by generation 3000)


@pytest.mark.parametrize("name", ["bool", "float16"])
def test_evolve(gol, name):
    glider = np.zeros((64, 64), np.uint8)
    glider[61:64, 61:64] = [[0, 1, 0], [0, 0, 1], [1, 1, 1]]  # four generations from crossing both seams
    x = torch.from_numpy(glider).to(f"cuda:{DEV}").to(tc.dt(name))
    y = gol.ops.evolve(x, 12)
    assert y.shape == x.shape and y.dtype == x.dtype and y.device == x.device
    ref = numpy_step_rule(glider, CONWAY, 12)
    assert ref[0:3, 0:3].sum() == 5 and ref.sum() == 5  # (the glider is through the corner)
    tc.assert_cells(y, name, ref)
    boards = np.stack([random_board(128, 128, 50 + i) for i in range(7)])
    boards[3] = 0
    boards[3, 125:128, 125:128] = [[0, 1, 0], [0, 0, 1], [1, 1, 1]]
    xb = torch.from_numpy(boards).to(f"cuda:{DEV}").to(tc.dt(name))
    yb = gol.ops.evolve(xb, 12, rule=CONWAY)
    assert yb.shape == xb.shape and yb.dtype == xb.dtype and yb.device == xb.device
    tc.assert_cells(yb, name, np.stack([numpy_step_rule(b, CONWAY, 12) for b in boards]))
    tc.assert_cells(xb, name, boards)  # (the input is left alone)


# ----- refusals on the device -----


def test_wrong_side_is_refused(gol):
    shape = (65, 70)
    h = _sim(gol, shape).init(5, seed=3)
    c = _sim(gol, shape, backend="cpu").init(5, seed=3)
    before = h.board()
    on_cpu = torch.ones(shape, dtype=torch.uint8)
    on_gpu = on_cpu.to(f"cuda:{DEV}")
    with pytest.raises(ValueError, match="on cpu"):
        h.load_tensor(on_cpu)
    with pytest.raises(ValueError, match="on cpu"):
        h.board_tensor(out=on_cpu)
    with pytest.raises(ValueError, match=f"on cuda:{DEV}"):
        c.load_tensor(on_gpu)
    with pytest.raises(ValueError, match=f"on cuda:{DEV}"):
        c.board_tensor(out=on_gpu)
    # behind the Python checks the HIP engine asks the runtime: a host pointer never reaches a kernel
    with pytest.raises(ValueError, match="not device memory|host or managed"):
        h.engine.write_tile_cells(on_cpu.data_ptr(), 0, on_cpu.numel())
    with pytest.raises(ValueError, match="not device memory|host or managed"):
        h.engine.read_tile_cells(on_cpu.data_ptr(), 0, on_cpu.numel())
    assert np.array_equal(h.board(), before) and np.array_equal(c.board(), before)
    assert bool((on_cpu == 1).all()) and bool((on_gpu == 1).all())
    with pytest.raises(ValueError, match="on cpu"):
        gol.SoupBatch(4, 64, backend="hip", device=DEV).boards_tensor(out=torch.empty((4, 64, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="backend 'cpu'"):
        gol.SoupBatch.from_tensor(on_gpu.new_zeros((2, 64, 64)), backend="cpu")
    h.step(2)  # (the engine is sound after the refusals)
    tc.assert_cells(h.board_tensor(), "uint8", tc_board(shape, 3, 2))


def tc_board(shape, seed, gens):
    return numpy_step_rule(random_board(shape[0], shape[1], seed), CONWAY, gens)
