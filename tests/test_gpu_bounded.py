"""Bounded boards (``boundary="dead"``) on the HIP backend: the kernel step_rule_bounded<K> (rule_bounded_kernel.hip)
under every engine path it takes -- pass depths, board sizes, wrap and ghost rows, multi-pass supersteps, graphs,
thread ranks, the 1-rank RCCL communicator, views and checkpoints -- bit for bit against the zero-padded numpy
oracle ``numpy_step_rule_bounded``.

Every comparison also asserts that the bounded oracle's result differs from the torus oracle's for its input
(where a board is large enough to tell them apart), so running the torus could not pass."""
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_step_rule, numpy_step_rule_bounded, random_board

pytestmark = pytest.mark.gpu

HIGHLIFE = "B36/S23"
# B1 rules put births just outside the board at every level of a pass: a mask missing at one level, or at the
# input, shows within the pass
RULES = ["B3/S23", HIGHLIFE, "B1357/S1357", "B1/S012345678"]
GLIDER_SE = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8)  # moves down and right


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    kw.setdefault("boundary", "dead")
    return gol.Simulation(N, **kw)


def oracle(board, rule, gens):
    """The bounded oracle's result, checked to differ from the torus oracle's on this input."""
    ref = numpy_step_rule_bounded(board, rule, gens)
    assert not np.array_equal(ref, numpy_step_rule(board, rule, gens)), "the input does not tell the boundaries apart"
    return ref


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sweep(gol, K, N):
    """Every pass depth on every size class (ROWS_WRAP on boards shorter than the pass, unaligned widths, packed
    narrow segments, several blocks): 2K + 1 generations, a full superstep and the remainders."""
    gens = 2 * K + 1
    board = initial_board(5, N, 1, True, N + K)
    told_apart = False
    for rule in RULES:
        s = _sim(gol, N, rule=rule, kernel="rule", halo_depth=K, kernel_depth=K).init(5, seed=N + K)
        st = s.stats()
        assert st["kernel"].startswith("rule@") and st["boundary"] == "dead", st
        s.step(gens)
        ref = numpy_step_rule_bounded(board, rule, gens)
        assert np.array_equal(s.board(), ref), (rule, N, K, int((s.board() != ref).sum()))
        told_apart = told_apart or not np.array_equal(ref, numpy_step_rule(board, rule, gens))
    assert told_apart or N <= 3  # (boards of 1 to 3 cells a side die out under either boundary)


@pytest.mark.parametrize("H,W", [(70, 130), (100, 200), (200, 64), (5, 1000)])
@pytest.mark.parametrize("rule", [HIGHLIFE, "B1/S012345678"])
def test_rectangular(gol, H, W, rule):
    """Unaligned rectangles, an aligned one-word board, and a strip shorter than the pass depth."""
    gens = 17
    s = _sim(gol, H, rule=rule, width=W, halo_depth=8).init(5, seed=5)
    assert s.stats()["kernel"].startswith("rule@"), s.stats()  # kernel auto resolves to the bounded rule kernel
    s.step(gens)
    board = random_board(H, W, 5)
    ref = oracle(board, rule, gens) if rule == HIGHLIFE else numpy_step_rule_bounded(board, rule, gens)
    assert np.array_equal(s.board(), ref)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("R", [16, 24])
@pytest.mark.parametrize("N", [137, 1000])
def test_multipass_supersteps(gol, N, R, graph):
    """Supersteps of two and three passes of 8: later passes read what earlier ones wrote."""
    gens = 37
    for rule in (HIGHLIFE, "B1/S012345678"):
        s = _sim(gol, N, rule=rule, halo_depth=R, kernel_depth=8, graph=graph).init(5, seed=6)
        st = s.stats()
        assert st["depth"] == R and st["kernel_depth"] == 8 and st["kernel"].startswith("rule@8"), st
        s.step(gens)
        st = s.stats()
        assert (st["graph_launches"] >= 1) if graph else (st["graph_launches"] == 0), st
        board = initial_board(5, N, 1, True, 6)
        ref = oracle(board, rule, gens) if rule == HIGHLIFE else numpy_step_rule_bounded(board, rule, gens)
        assert np.array_equal(s.board(), ref), rule


def test_conway_runs_the_bounded_rule_kernel(gol):
    """B3/S23 too: kernel auto is the bounded rule kernel, and the torus-only kernels are refused."""
    N, gens = 256, 45
    s = _sim(gol, N, halo_depth=8).init(5, seed=9)
    assert s.stats()["kernel"].startswith("rule@") and s.stats()["rule"] == "B3/S23", s.stats()
    assert s.describe().endswith(", boundary dead")
    s.step(gens)
    assert np.array_equal(s.board(), oracle(initial_board(5, N, 1, True, 9), "B3/S23", gens))
    for kernel in ("temporal", "tile", "pipe", "resident", "lds"):
        with pytest.raises(ValueError) as e:
            _sim(gol, N, kernel=kernel)
        assert "torus only" in str(e.value)
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.boundary, cfg.kernel, cfg.device = "hip", "dead", kernel, 0
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(s.geometry, cfg, s.transport)
        assert f"kernel '{kernel}' implements the torus only" in str(e.value)


@pytest.mark.parametrize("H,W", [(64, 64), (100, 130)])
def test_gliders_leave(gol, H, W):
    """A glider 2 cells from each of the four edges, heading out: against the oracle, and no live cell ever
    appears in the opposite third of the board."""
    for name, pat, at in [("bottom-right", GLIDER_SE, (H - 5, W - 5)), ("top-left", GLIDER_SE[::-1, ::-1], (2, 2)),
                          ("top-right", GLIDER_SE[::-1, :], (2, W - 5)), ("bottom-left", GLIDER_SE[:, ::-1], (H - 5, 2))]:
        s = _sim(gol, H, width=W, halo_depth=8).init(0)
        s.stamp(pat, at=at)
        start = s.board()
        far_r = slice(0, H // 3) if at[0] > H // 2 else slice(H - H // 3, H)
        far_c = slice(0, W // 3) if at[1] > W // 2 else slice(W - W // 3, W)
        for _ in range(8):
            s.step(8)
            b = s.board()
            assert b[far_r, :].sum() == 0 and b[:, far_c].sum() == 0, name
        assert s.generation == 64
        assert np.array_equal(s.board(), oracle(start, "B3/S23", 64)), name


def _thread_ranks(gol, P, N, gens, rule, **kw):
    """P ranks as threads on one GPU (p2p emulation); the global board, from the HIP and from the CPU backend."""
    out = {}
    for backend in ("hip", "cpu"):
        ts = gol.parallel.p2p_thread_transports(P) if backend == "hip" else gol.parallel.thread_transports(P)
        parts, errs = [None] * P, []

        def rank_main(r):
            try:
                extra = {"device": 0} if backend == "hip" else {}
                s = gol.Simulation(N, ts[r], backend=backend, global_mode=True, rule=rule, boundary="dead", **extra, **kw)
                s.init(5, seed=17)
                if backend == "hip":
                    assert s.stats()["kernel"].startswith("rule@"), s.stats()
                s.step(gens)
                parts[r] = (s.geometry.row0, s.geometry.col0, s.board())
            except Exception as e:  # pragma: no cover - reported below
                errs.append(repr(e))

        th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs
        full = np.zeros((N, N), np.uint8)
        for r0, c0, b in parts:
            full[r0 : r0 + b.shape[0], c0 : c0 + b.shape[1]] = b
        out[backend] = full
    return out


@pytest.mark.parametrize("P,kw", [(2, {"schedule": "split"}), (3, {"schedule": "full"}), (4, {}),
                                  (4, {"decomp": "2d", "grid": "2x2"})], ids=["P2-split", "P3-full", "P4", "2x2"])
def test_thread_ranks(gol, P, kw):
    """The torus exchanges keep running between the edge ranks; what they deliver is masked away."""
    N, gens = 256, 40
    board = initial_board(5, N, 1, True, 17)
    for rule in (HIGHLIFE, "B1/S012345678"):
        got = _thread_ranks(gol, P, N, gens, rule, halo_depth=16, **kw)
        ref = oracle(board, rule, gens) if rule == HIGHLIFE else numpy_step_rule_bounded(board, rule, gens)
        assert np.array_equal(got["hip"], ref), rule
        assert np.array_equal(got["cpu"], ref), rule


@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


@pytest.mark.parametrize("kw", [{}, {"decomp": "2d"}], ids=["1d", "2d"])
def test_rccl_self(gol, rccl, kw):
    """Every halo path of the multi-GPU engine on one rank: the rank is its own wrap-around neighbour, and all it
    receives lies beyond the board."""
    N, R, gens = 256, 8, 40
    board = initial_board(5, N, 1, True, R)
    for rule in (HIGHLIFE, "B1/S012345678"):
        s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=rule, boundary="dead", halo_depth=R,
                           subtiles=0, **kw)
        s.init(5, seed=R)
        s.step(gens)
        st = s.stats()
        got = s.board()
        s.synchronize()
        assert st["kernel"].startswith("rule@") and st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
        ref = oracle(board, rule, gens) if rule == HIGHLIFE else numpy_step_rule_bounded(board, rule, gens)
        assert np.array_equal(got, ref), rule


def test_views(gol):
    """window, density and stamp inside the board are what they are on the torus; a rectangle across an edge raises."""
    N, W = 70, 130
    s = _sim(gol, N, width=W, rule=HIGHLIFE, halo_depth=8).init(5, seed=3)
    s.step(5)
    ref = oracle(random_board(N, W, 3), HIGHLIFE, 5)
    assert np.array_equal(s.window(0, 0, N, W), ref)
    assert np.array_equal(s.window(60, 100, 10, 30), ref[60:70, 100:130])
    dens = s.density(32, 64)
    assert dens.shape == (3, 3) and int(dens.sum()) == int(ref.sum()) and dens[2, 2] == ref[64:, 128:].sum()
    assert s.population() == int(ref.sum())
    for rect in [(-1, 0, 5, 5), (0, -1, 5, 5), (66, 0, 5, 5), (0, 126, 5, 5)]:
        with pytest.raises(ValueError) as e:
            s.window(*rect)
        assert "bounded" in str(e.value)
        with pytest.raises(gol.native.GolError) as e:
            s.engine.window(*rect)
        assert "bounded" in str(e.value)
        with pytest.raises(ValueError):
            s.stamp(np.ones((5, 5), np.uint8), at=rect[:2])
        with pytest.raises(gol.native.GolError):
            s.engine.stamp(gol.ops.pattern_from_cells(np.ones((5, 5), np.uint8)), rect[0], rect[1], "or")
    # stamps in the last word's partial cells and in the last rows, then a step
    s.init(0).stamp(np.ones((3, 3), np.uint8), at=(67, 127))
    start = np.zeros((N, W), np.uint8)
    start[67:70, 127:130] = 1
    assert np.array_equal(s.board(), start)
    s.stamp(GLIDER_SE, at=(0, 0), mode="xor")
    start[0:3, 0:3] ^= GLIDER_SE
    s.step(9)
    assert np.array_equal(s.board(), oracle(start, HIGHLIFE, 9))


def test_checkpoint_round_trip(gol, tmp_path):
    N, gens = 137, 11
    s = _sim(gol, N, halo_depth=8).init(5, seed=4)
    s.step(gens)
    s.checkpoint(str(tmp_path / "d"))
    again = _sim(gol, N, halo_depth=8).init(0)
    assert again.restore(str(tmp_path / "d")) == gens
    again.step(5)
    assert np.array_equal(again.board(), oracle(initial_board(5, N, 1, True, 4), "B3/S23", gens + 5))
    torus = _sim(gol, N, boundary="torus", halo_depth=8).init(0)
    with pytest.raises(gol.native.GolError) as e:
        torus.restore(str(tmp_path / "d"))
    assert "boundary dead" in str(e.value) and "boundary torus" in str(e.value)
