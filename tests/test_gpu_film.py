"""Film mode on the HIP backend: the kernel step_film<K> (film_kernel.hip, nbhd_film_kernel.hip) under every schedule
the census kernel runs under -- pass depths, board sizes, wrap and ghost rows, both boundaries, window shapes, wide
boards with full-width segments, multi-pass supersteps, a frame buffer forced small, thread ranks sharing the GPU, rank
grids, the 1-rank RCCL communicator, the other neighbourhoods -- against the numpy oracle ``numpy_film``.

Every comparison is exact, and each also asserts the ``film@`` kernel, ``stats()["film"]`` and that the final board is
the oracle's (film_cases.check).  Random boards keep the ghost rows and words live, so a frame that holds a redundantly
computed cell, or misses an owned one, is wrong."""
import numpy as np
import pytest

import film_cases as fc
import wide_cases as wc
from gol_amd.ops import numpy_film, random_board

pytestmark = pytest.mark.gpu


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


def test_depths_are_instantiated(gol):
    assert gol.native.max_film_depth() == 8


@pytest.mark.parametrize("N", fc.SIZES)
@pytest.mark.parametrize("K", fc.DEPTHS)
def test_sweep(gol, K, N):
    """Every pass depth on every size class (wrap rows on boards shorter than the pass, where one owned row is computed
    many times; tail words of 1, 63 and 9 cells; packed segments in the per-lane runner; several blocks); the window is
    the whole board, on the torus across both seams."""
    fc.run_sweep_case(lambda n, **kw: _sim(gol, n, **kw), K, N, kernel="film@")  # (a 1-, 2- or 3-row board clamps the depth)


@pytest.mark.parametrize("K", [8, 3])
@pytest.mark.parametrize("name", list(fc.WINDOWS))
def test_window_shapes(gol, name, K):
    fc.run_window_case(lambda n, **kw: _sim(gol, n, **kw), name, K, kernel=f"film@{K}")


# (shape, rows_per_wave, window).  64 x 4096: columns 3960 .. 4039, words 61 to 63 (lanes 62 and 63 of the full-width
# segment and the packed two-word remainder), rows wrapping.  50 x 3969: the x seam through the one-cell tail word.
# 48 x 8000: columns 3900 .. 4050, the seam between full-width segments.  600 x 4096 in 300-row segments: rows 290 .. 310.
# On a bounded board a window that wraps is moved inside (the same words: it keeps its last column or row).
WIDE = [
    (wc.S4096, 0, (60, 3960, 10, 80)),
    (wc.S3969, 0, (45, 3900, 10, 140)),
    (wc.S8000, 0, (0, 3900, 48, 151)),
    (wc.TALL, wc.TALL_ROWS, (290, 4000, 21, 96)),
]


@pytest.mark.parametrize("shape,rows,rect", WIDE, ids=[wc.shape_id(s) for s, _, _ in WIDE])
@pytest.mark.parametrize("K", [5, 8])
def test_wide(gol, K, shape, rows, rect):
    """Full-width segments in the scalar runner (wide_cases.py tells what each shape gives)."""
    gens = 2 * K + 1
    H, W = shape.H, shape.W
    torus_rect = rect
    for boundary in fc.BOUNDARIES:
        rect = torus_rect
        if boundary == "dead":
            rect = (min(rect[0], H - rect[2]), min(rect[1], W - rect[3]), rect[2], rect[3])
        rule = fc.HIGHLIFE
        ref = fc.frames_of(H, W, wc.SEED, rule, boundary, wc.SWEEP_GENS, rect)[:gens]
        board = wc.board_after(shape, rule, boundary, gens)
        assert len({f.tobytes() for f in ref}) >= 2
        s = _sim(gol, H, width=W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, rows_per_wave=rows,
                 film=rect).init(5, seed=wc.SEED)
        s.step(gens)
        fc.check(s, 0, ref, board, rect, f"film@{K}")


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("boundary", fc.BOUNDARIES)
@pytest.mark.parametrize("passes", [2, 3])
def test_multipass_supersteps(gol, passes, boundary, graph):
    """Supersteps of two and three passes of depth 8 plus a remainder: the extension rows the earlier passes compute
    beyond the tile are not stored; launches are eager whatever GOL_GRAPH says."""
    N, R, gens, seed = 137, 8 * passes, 37, 6
    rect = fc.sweep_rect(N, boundary)
    for rule in fc.RULES:
        s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=R, kernel_depth=8, graph=bool(graph), film=rect).init(5, seed=seed)
        st = s.stats()
        assert st["depth"] == R and st["kernel_depth"] == 8, st
        s.step(gens)
        assert s.stats()["graph_launches"] == 0
        assert fc.lively(N, N, seed, rule, boundary, gens, rect)
        fc.check(s, 0, fc.frames_of(N, N, seed, rule, boundary, gens, rect), fc.boards_of(N, N, seed, rule, boundary, gens)[-1],
                 rect, "film@8")


def test_several_steps_clear_init_restore(gol, tmp_path):
    """Several step() calls around a stamp(), film_clear(), checkpoint() / restore() and init(); start every time."""
    N, rule, rect, seed = 137, fc.HIGHLIFE, (100, 120, 50, 40), 8
    s = _sim(gol, N, rule=rule, halo_depth=8, film=rect).init(5, seed=seed)
    assert s.film()[0] == 0 and s.film()[1].shape == (0, 50, 40)  # (the init-time timing launches left nothing)
    ref = fc.frames_of(N, N, seed, rule, "torus", 29, rect)
    boards = fc.boards_of(N, N, seed, rule, "torus", 29)
    s.step(5).step(20).step(1)
    fc.check(s, 0, ref[:26], boards[25], rect, "film@8")
    s.film_clear()
    assert s.film()[0] == 26 and len(s.film()[1]) == 0
    s.step(3)
    fc.check(s, 26, ref[26:], boards[28], rect)
    s.stamp(np.ones((3, 3), np.uint8), at=(110, 130), mode="xor")  # (leaves the record running)
    b = s.board()
    s.step(4)
    start, got = s.film()
    assert start == 26 and len(got) == 7 and np.array_equal(got[:3], ref[26:])
    assert np.array_equal(got[3:], numpy_film(b, rule, 4, rect))
    s.checkpoint(str(tmp_path / "ck"))
    s.step(2)
    assert s.restore(str(tmp_path / "ck")) == 33
    assert s.film()[0] == 33 and len(s.film()[1]) == 0
    s.step(5)
    start, got = s.film()
    assert start == 33 and np.array_equal(got, numpy_film(numpy_film(b, rule, 4, (0, 0, N, N))[-1], rule, 5, rect))
    s.init(5, seed=seed)
    s.step(7)
    fc.check(s, 0, ref[:7], boards[6], rect)


def test_small_buffer_chunks(gol, monkeypatch):
    """GOL_FILM_MB=1: a frame of the 600 x 1000 window (16 words a row) takes 76800 bytes, the buffer holds 13 of them,
    and 40 generations take four chunks.  A window of which fewer than 8 frames fit is refused at init."""
    monkeypatch.setenv("GOL_FILM_MB", "1")
    N, gens, rule, rect = 1000, 40, fc.HIGHLIFE, (700, 30, 600, 1000)
    fw = 16
    per_chunk = (1 << 20) // (rect[2] * fw * 8)
    assert 8 <= per_chunk and -(-gens // per_chunk) >= 3
    s = _sim(gol, N, rule=rule, halo_depth=16, kernel_depth=8, film=rect).init(5, seed=2)
    s.step(gens)
    ref, last = numpy_film(random_board(N, N, 2), rule, gens, rect, return_board=True)
    assert len({f.tobytes() for f in ref}) >= 2
    fc.check(s, 0, ref, last, rect, "film@8")
    monkeypatch.setenv("GOL_FILM_MB", "1")
    with pytest.raises(gol.native.GolError) as e:  # fewer than 8 frames fit
        _sim(gol, 2048, rule=rule, film=(0, 0, 2048, 2048))
    assert "GOL_FILM_MB" in str(e.value)


@pytest.mark.parametrize("boundary", fc.BOUNDARIES)
def test_same_frames_as_step_window_loop(gol, boundary):
    N, gens, rule = 200, 21, fc.HIGHLIFE
    rect = (150, 170, 80, 90) if boundary == "torus" else (100, 110, 80, 90)
    a = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=8, film=rect).init(5, seed=4)
    b = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=8).init(5, seed=4)
    a.step(gens)
    loop = []
    for _ in range(gens):
        b.step(1)
        loop.append(b.window(*rect))
    start, got = a.film()
    assert start == 0 and np.array_equal(got, np.stack(loop)) and len({f.tobytes() for f in got}) >= 2
    assert np.array_equal(a.board(), b.board())


@pytest.mark.parametrize("boundary", fc.BOUNDARIES)
@pytest.mark.parametrize("name,kw", [("1d4", {"schedule": "split"}), ("1d4", {"schedule": "full"}), ("2x2", {}), ("3x3", {})],
                         ids=["P4-split", "P4-full", "2x2", "3x3"])
def test_thread_ranks(gol, name, kw, boundary):
    """Thread ranks on hip and on cpu against numpy: strips under the split and the full schedule, a 2 x 2 grid with a
    window over the point where the four tiles meet, a 3 x 3 grid with a window over nine ranks and one inside the centre
    rank (eight ranks run the kernel and store nothing).  Supersteps of two passes and remainders; every rank gets every
    frame."""
    P, grid, H, W, _ = fc.RANK_CASES[name]
    rule = fc.HIGHLIFE
    for rect in fc.rank_windows(name, boundary):
        ref, board = fc.rank_ref(name, rule, boundary, rect)
        assert fc.distinct(H, W, fc.RANK_SEED, rule, boundary, fc.RANK_GENS, rect)
        assert boundary == "torus" or fc.told_apart(H, W, fc.RANK_SEED, rule, fc.RANK_GENS, (0, 0, H, W))
        for backend in ("hip", "cpu"):
            parts = wc.run_ranks(gol, P, H, W, backend, script=fc.film_script, rule=rule, boundary=boundary, film=rect,
                                 **grid, **kw)
            assert np.array_equal(wc.assemble(H, W, parts), board), backend
            for p in parts:
                start, frames, st = p.result
                assert start == 0 and st["film"] == rect and np.array_equal(frames, ref), (backend, p.rank)
                if backend == "hip":
                    assert st["kernel"].startswith("film@"), st
                    if "schedule" in kw:
                        assert ("+boundary:film@" in st["kernel"]) == (kw["schedule"] == "split"), st


@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


@pytest.mark.parametrize("boundary", fc.BOUNDARIES)
@pytest.mark.parametrize("kw", [{}, {"decomp": "2d"}], ids=["1d", "2d"])
def test_rccl_self(gol, rccl, kw, boundary):
    N, R, gens, rule = 256, 16, 40, fc.HIGHLIFE
    rect = fc.sweep_rect(N, boundary)
    s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=rule, boundary=boundary, halo_depth=R,
                       kernel_depth=8, subtiles=0, film=rect, **kw)
    s.init(5, seed=R)
    s.step(gens)
    st = s.stats()
    assert st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
    assert fc.lively(N, N, R, rule, boundary, gens, rect)
    fc.check(s, 0, fc.frames_of(N, N, R, rule, boundary, gens, rect), fc.boards_of(N, N, R, rule, boundary, gens)[-1], rect,
             "film@8")
    s.synchronize()


@pytest.mark.parametrize("boundary", fc.BOUNDARIES)
@pytest.mark.parametrize("K", [8, 3])
@pytest.mark.parametrize("rule", ["B13/S13V", "B2/S34H"])
def test_neighbourhoods(gol, rule, K, boundary):
    N, gens, seed = 137, 2 * K + 3, 12
    rect = fc.sweep_rect(N, boundary)
    assert fc.lively(N, N, seed, rule, boundary, gens, rect)
    s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, film=rect).init(5, seed=seed)
    s.step(gens)
    fc.check(s, 0, fc.frames_of(N, N, seed, rule, boundary, gens, rect), fc.boards_of(N, N, seed, rule, boundary, gens)[-1], rect,
             f"film@{K}")


def test_run_hint_prediction_leaves_no_frame(gol):
    N, gens, rule, rect = 200, 21, fc.HIGHLIFE, (190, 10, 30, 100)
    s = _sim(gol, N, rule=rule, halo_depth=8, run_hint=gens, film=rect).init(5, seed=3)
    assert s.generation == 0 and len(s.film()[1]) == 0
    s.step(gens)
    fc.check(s, 0, fc.frames_of(N, N, 3, rule, "torus", gens, rect), fc.boards_of(N, N, 3, rule, "torus", gens)[-1], rect, "film@8")


def test_refusals(gol):
    ok = (0, 0, 8, 8)
    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"compat": True}, "compat"),
                     ({"subtiles": 2}, "subtiles=2"), ({"kernel_depth": 9}, "kernel_depth 9")] + [
                         ({"kernel": k}, k) for k in ("temporal", "tile", "pipe", "resident", "lds")]:
        with pytest.raises(ValueError) as e:
            _sim(gol, 64, film=ok, **kw)
        assert word in str(e.value) and "film" in str(e.value), str(e.value)
    for rect, boundary, word in [((0, 0, 65, 8), "torus", "1..64"), ((60, 0, 8, 8), "dead", "inside the bounded 64 x 64"),
                                 ((0, 0, 2049, 2048), "torus", "2^22")]:
        with pytest.raises(ValueError) as e:
            _sim(gol, 64 if rect[2] <= 65 else 4096, film=rect, boundary=boundary)
        assert word in str(e.value), str(e.value)
    # the engine on its own refuses the same
    dec = gol.native.make_decomposition(64, 1, False, "1d", "", 0)
    geo = gol.native.make_geometry(dec, 0)
    for attr, value, word in [("kernel_depth", 9, "kernel_depth 9"), ("kernel", "temporal", "temporal"), ("kernel", "lds", "lds"),
                              ("census", True, "census"), ("boundary", "dead", "bounded 64 x 64")]:
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.device = "hip", 0
        cfg.film = (60, 60, 8, 8) if attr == "boundary" else ok
        setattr(cfg, attr, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
        assert word in str(e.value), str(e.value)
