"""Windows, density maps and pattern stamping on the HIP backend (view_kernels.hip): every comparison is bit for
bit against numpy on ``board()`` / ``initial_board``.  Small boards, where the kernels can still go wrong:
unaligned widths (the tile's last word has 1..63 valid bits, the ghost word sits next to it), windows and
patterns across the seams, every stepping kernel and schedule around a stamp, thread ranks, a 1-rank RCCL
communicator."""
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_step, numpy_step_rule, random_board

pytestmark = pytest.mark.gpu

HIGHLIFE = "B36/S23"
MODES = ["or", "replace", "xor", "clear"]


def np_window(board, r0, c0, rows, cols):
    return np.take(np.take(board, np.arange(r0, r0 + rows), axis=0, mode="wrap"), np.arange(c0, c0 + cols), axis=1,
                   mode="wrap")


def np_density(board, br, bc):
    H, W = board.shape
    gh, gw = -(-H // br), -(-W // bc)
    pad = np.zeros((gh * br, gw * bc), np.uint32)
    pad[:H, :W] = board
    return pad.reshape(gh, br, gw, bc).sum(axis=(1, 3)).astype(np.uint32)


def np_stamp(board, pat, r0, c0, mode):
    out = board.copy()
    idx = np.ix_((r0 + np.arange(pat.shape[0])) % board.shape[0], (c0 + np.arange(pat.shape[1])) % board.shape[1])
    cur = out[idx]
    out[idx] = {"or": cur | pat, "replace": pat, "xor": cur ^ pat, "clear": cur & (1 - pat)}[mode]
    return out


def rand_cells(rows, cols, seed, density=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < density).astype(np.uint8)


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


def _window(s, board, r0, c0, rows, cols):
    """window() against numpy; exactly the window's bytes crossed to the host."""
    before = s.stats()["view_bytes_d2h"]
    got = s.window(r0, c0, rows, cols)
    assert s.stats()["view_bytes_d2h"] - before == rows * cols, (r0, c0, rows, cols)
    assert got.dtype == np.uint8 and got.shape == (rows, cols)
    assert np.array_equal(got, np_window(board, r0, c0, rows, cols)), (r0, c0, rows, cols)


@pytest.mark.parametrize("N,W", [(1, 0), (3, 0), (63, 0), (64, 0), (65, 0), (127, 0), (137, 0), (200, 0), (100, 200)])
def test_windows_and_density(gol, N, W):
    s = _sim(gol, N, width=W, halo_depth=8).init(5, seed=N)
    board = random_board(N, W or N, N)
    H, Wd = board.shape
    assert np.array_equal(s.board(), board)
    wins = [(0, 0, 1, 1), (H - 1, Wd - 1, 1, 1), (0, 0, H, Wd), (H // 2, Wd // 2, H, Wd),
            (H - 1, 2, min(H, 2), 1),                      # the row seam only
            (1, Wd - 1, 1, min(Wd, 2)),                    # the column seam only
            (-1, -1, min(H, 3), min(Wd, 3)),               # both
            (3 * H + 1, -2 * Wd + 2, max(1, H - 1), max(1, Wd - 1))]
    if Wd >= 71:
        wins += [(2, 63, 3, 2), (0, 60, H, 11), (H - 2, 60, 4, 11)]  # columns 63..64 and 60..70
    for win in wins:
        _window(s, board, *win)
    for br, bc in [(1, 64), (7, 64), (64, 128), (H, 64 * -(-Wd // 64))]:
        got = s.density(br, bc)
        assert got.dtype == np.uint32 and np.array_equal(got, np_density(board, br, bc)), (br, bc)
    # after a few generations too (the board has changed buffers)
    s.step(5)
    board = s.board()
    _window(s, board, H // 2, Wd // 2, H, Wd)
    assert np.array_equal(s.density(7, 64), np_density(board, 7, 64))
    assert int(s.density(64).sum()) == s.population() == int(board.sum())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [137, 192])
def test_stamp_modes(gol, mode, N):
    """A seeded random 37 x 70 pattern at offsets 0, 1, 63, 64 and across both seams; after each stamp 9
    generations against numpy_step of the numpy-stamped board (stale ghost cells or halos would show)."""
    pat = rand_cells(37, 70, seed=3)
    s = _sim(gol, N, halo_depth=8).init(5, seed=N)
    board = initial_board(5, N, 1, True, N)
    for at in [(0, 0), (1, 1), (63, 63), (64, 64), (0, 63), (N - 10, N - 20), (N - 1, 64)]:
        s.stamp(pat, at=at, mode=mode)
        board = np_stamp(board, pat, at[0], at[1], mode)
        assert np.array_equal(s.board(), board), at
        s.step(9)
        board = numpy_step(board, 9)
        assert np.array_equal(s.board(), board), at


def test_stamp_small_and_exact_fit(gol):
    """A pattern exactly the board's size (it wraps onto every cell once), on a board of one word and less."""
    for N, W in [(37, 70), (5, 3), (1, 1)]:
        pat = rand_cells(N, W, seed=N)
        s = _sim(gol, N, width=W, halo_depth=4).init(5, seed=2)
        board = random_board(N, W, 2)
        for mode, at in zip(MODES, [(0, 0), (N - 1, W - 1), (N // 2, 1), (1, W // 2)]):
            s.stamp(pat, at=at, mode=mode)
            board = np_stamp(board, pat, at[0], at[1], mode)
            assert np.array_equal(s.board(), board), (N, W, mode)
        s.step(5)
        assert np.array_equal(s.board(), numpy_step(board, 5))
    with pytest.raises((ValueError, gol.native.GolError)):
        s.stamp(np.ones((2, 1), np.uint8))
    with pytest.raises(gol.native.GolError) as e:
        s.engine.stamp(gol.ops.pattern_from_cells(np.ones((2, 1), np.uint8)), 0, 0, "or")
    assert "larger than the board" in str(e.value)
    with pytest.raises(gol.native.GolError):
        s.engine.density(1, 100)


@pytest.mark.parametrize("kw", [{"kernel": "temporal", "graph": False}, {"kernel": "temporal", "graph": True},
                                {"kernel": "tile"}, {"kernel": "rule", "rule": HIGHLIFE}, {"kernel": "resident"}],
                         ids=["temporal", "temporal-graph", "tile", "rule-highlife", "resident"])
def test_around_the_kernels(gol, kw):
    """step -> window -> stamp -> step under each stepping kernel, eager and through graph replays."""
    N, R = 256, 8
    rule = kw.get("rule", "B3/S23")
    pat = rand_cells(37, 70, seed=4)
    s = _sim(gol, N, halo_depth=R, kernel_depth=R, subtiles=0, **kw).init(5, seed=21)
    gens = R * 20 + 3
    s.step(gens)
    board = numpy_step_rule(initial_board(5, N, 1, True, 21), rule, gens)
    _window(s, board, N - 5, N - 9, 40, 70)
    assert np.array_equal(s.density(64, 64), np_density(board, 64, 64))
    s.stamp(pat, at=(N - 11, N - 33), mode="xor")
    board = np_stamp(board, pat, N - 11, N - 33, "xor")
    _window(s, board, 0, 0, N, N)
    s.step(gens)
    board = numpy_step_rule(board, rule, gens)
    assert np.array_equal(s.board(), board)
    if kw.get("graph"):
        assert s.stats()["graph_launches"] >= 2, s.stats()


def test_subtiles(gol):
    """Two sub-tiles per rank: a reader first copies the halves back to the canonical board, a stamp edits it
    and the halves reload at the next run."""
    N, R = 640, 8
    pat = rand_cells(37, 70, seed=5)
    s = _sim(gol, N, halo_depth=R, kernel="temporal", subtiles=2).init(5, seed=N + R)
    assert "subtiles2" in s.stats()["schedule"], s.stats()
    s.step(R * 3 + 1)
    board = numpy_step(initial_board(5, N, 1, True, N + R), R * 3 + 1)
    _window(s, board, N // 2 - 20, N - 30, 40, 70)  # across the seam between the halves, and the column seam
    assert np.array_equal(s.density(64, 128), np_density(board, 64, 128))
    s.step(7)
    board = numpy_step(board, 7)
    s.stamp(pat, at=(N // 2 - 18, N - 35), mode="replace")
    board = np_stamp(board, pat, N // 2 - 18, N - 35, "replace")
    s.step(R * 2 + 5)
    board = numpy_step(board, R * 2 + 5)
    _window(s, board, 0, 0, N, N)
    assert np.array_equal(s.board(), board)


def _thread_views(gol, P, **kw):
    N = 192  # the global board
    pat = rand_cells(37, 45, seed=5)
    at, win, mid = (N - 10, N - 20), (N - 30, N - 25, 70, 50), (N // 2 - 30, N // 2 - 20)
    ts = gol.parallel.p2p_thread_transports(P)
    out, errs = [None] * P, []

    def script(s):
        s.init(5, seed=11)
        s.step(3)
        res = {"w0": s.window(*win), "d0": s.density(7, 64), "full0": s.window(0, 0, N, N)}
        s.stamp(pat, at=at, mode="xor")
        s.stamp(pat, at=mid, mode="replace")
        res["full1"] = s.window(0, 0, N, N)
        s.step(9)
        res["full2"] = s.window(N // 2, N // 2, N, N)
        res["d2"] = s.density(64, 64)
        return res

    def rank_main(r):
        try:
            out[r] = script(gol.Simulation(N, ts[r], backend="hip", device=0, global_mode=True, halo_depth=4, **kw))
        except Exception as e:  # pragma: no cover - reported below
            errs.append(repr(e))

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th) and not errs, errs
    cpu = script(gol.Simulation(N, backend="cpu"))
    for r in range(P):  # every rank holds the full result, and it is the CPU backend's
        for key in cpu:
            assert np.array_equal(out[r][key], cpu[key]), (r, key)
    b0 = numpy_step(initial_board(5, N, 1, True, 11), 3)
    b1 = np_stamp(np_stamp(b0, pat, at[0], at[1], "xor"), pat, mid[0], mid[1], "replace")
    b2 = numpy_step(b1, 9)
    assert np.array_equal(cpu["full0"], b0) and np.array_equal(cpu["w0"], np_window(b0, *win))
    assert np.array_equal(cpu["d0"], np_density(b0, 7, 64)) and np.array_equal(cpu["full1"], b1)
    assert np.array_equal(cpu["full2"], np_window(b2, N // 2, N // 2, N, N))
    assert np.array_equal(cpu["d2"], np_density(b2, 64, 64))


def test_thread_ranks_1d(gol):
    _thread_views(gol, 3)


def test_thread_ranks_2x2(gol):
    _thread_views(gol, 4, decomp="2d", grid="2x2")


def test_rccl_self_2d(gol):
    """The 2-D halo layout through a 1-rank RCCL communicator: a stamp across the seams, whose cells reach the
    other side only through the exchanged halos, then steps."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    N, R = 640, 8
    pat = rand_cells(37, 70, seed=6)
    s = gol.Simulation(N, t, backend="hip", device=0, self_exchange=True, halo_depth=R, decomp="2d").init(5, seed=R)
    s.step(R + 3)
    board = numpy_step(initial_board(5, N, 1, True, R), R + 3)
    s.stamp(pat, at=(N - 20, N - 40), mode="or")
    board = np_stamp(board, pat, N - 20, N - 40, "or")
    _window(s, board, N - 25, N - 45, 50, 90)
    s.step(3 * R + 2)
    board = numpy_step(board, 3 * R + 2)
    got = s.board()
    st = s.stats()
    s.synchronize()
    assert st["exchanges"] >= 4, st
    assert np.array_equal(got, board)
