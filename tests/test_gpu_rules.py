"""Life-like rules on the HIP backend: the generic kernel step_rule<K> (rule_kernel.hip) under every engine
path it takes -- pass depths, board sizes, wrap and ghost rows, multi-pass supersteps, graphs, thread ranks,
the 1-rank RCCL communicator -- bit for bit against the numpy oracle ``numpy_step_rule``."""
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_step_rule, random_board

pytestmark = pytest.mark.gpu

HIGHLIFE, DAYNIGHT = "B36/S23", "B3678/S34678"
SINGLE_BIT = [f"B{c}/S" for c in range(1, 9)] + [f"B/S{c}" for c in range(9)]


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


def neighbour_pairs(board):
    b = board.astype(np.int64)
    n = sum(np.roll(np.roll(b, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
    return np.array([[int(((b == s) & (n == c)).sum()) for c in range(9)] for s in (0, 1)])


@pytest.fixture(scope="module")
def board128():
    return initial_board(5, 128, 1, True, 1)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_depths(gol, K):
    N, gens = 192, 37
    s = _sim(gol, N, rule=HIGHLIFE, halo_depth=K, kernel_depth=K).init(5, seed=K)
    st = s.stats()
    assert st["kernel"].startswith("rule@") and st["kernel_depth"] == K and st["rule"] == HIGHLIFE, st
    s.step(gens)
    assert np.array_equal(s.board(), numpy_step_rule(initial_board(5, N, 1, True, K), HIGHLIFE, gens))


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000])
def test_board_sizes(gol, N):
    """ROWS_WRAP, tiles shorter than the halo, unaligned widths with ghost columns."""
    gens = 11
    s = _sim(gol, N, rule=DAYNIGHT, halo_depth=8).init(5, seed=N)
    assert s.stats()["kernel"].startswith("rule@"), s.stats()
    s.step(gens)
    assert np.array_equal(s.board(), numpy_step_rule(initial_board(5, N, 1, True, N), DAYNIGHT, gens))


@pytest.mark.parametrize("rule", SINGLE_BIT)
def test_single_bit_rules(gol, board128, rule):
    """Every entry of the rule table on its own; the board holds each (state, count) pair >= 25 times."""
    assert neighbour_pairs(board128).min() >= 25, neighbour_pairs(board128)
    s = _sim(gol, 128, rule=rule).init(5, seed=1)
    s.step(1)
    assert np.array_equal(s.board(), numpy_step_rule(board128, rule, 1))


def test_rectangular(gol):
    N, W, gens = 100, 200, 21
    s = _sim(gol, N, rule=HIGHLIFE, width=W, halo_depth=8).init(5, seed=5)
    s.step(gens)
    assert np.array_equal(s.board(), numpy_step_rule(random_board(N, W, 5), HIGHLIFE, gens))


def test_multipass_supersteps(gol):
    N, gens = 640, 32 * 2 + 5
    s = _sim(gol, N, rule=HIGHLIFE, halo_depth=32, kernel_depth=8).init(5, seed=6)
    st = s.stats()
    assert st["depth"] == 32 and st["kernel_depth"] == 8 and st["kernel"].startswith("rule@8"), st
    s.step(gens)
    assert np.array_equal(s.board(), numpy_step_rule(initial_board(5, N, 1, True, 6), HIGHLIFE, gens))


@pytest.mark.parametrize("graph", [True, False])
def test_graph_replay(gol, graph):
    N, gens = 512, 8 * 40 + 5
    s = _sim(gol, N, rule=HIGHLIFE, halo_depth=8, kernel_depth=8, graph=graph).init(5, seed=8)
    s.step(gens)
    st = s.stats()
    assert (st["graph_launches"] >= 1) if graph else (st["graph_launches"] == 0), st
    assert np.array_equal(s.board(), numpy_step_rule(initial_board(5, N, 1, True, 8), HIGHLIFE, gens))


def test_conway_through_generic_kernel(gol):
    """B3/S23 forced through step_rule equals the specialised step_temporal word for word."""
    N, gens = 512, 45
    a = _sim(gol, N, rule="B3/S23", kernel="rule", halo_depth=8).init(5, seed=9)
    b = _sim(gol, N, kernel="temporal", halo_depth=8).init(5, seed=9)
    assert a.stats()["kernel"].startswith("rule@") and b.stats()["kernel"].startswith("temporal"), (a.stats(), b.stats())
    a.step(gens)
    b.step(gens)
    assert np.array_equal(a.words(), b.words())


def test_kernel_selection(gol):
    s = _sim(gol, 256, rule=HIGHLIFE, kernel="auto").init(5, seed=2)
    assert s.stats()["kernel"].startswith("rule@"), s.stats()
    with pytest.raises(Exception) as e:
        _sim(gol, 256, rule=HIGHLIFE, kernel="tile")
    assert "tile" in str(e.value) and HIGHLIFE in str(e.value)
    # the native engine names both on its own too
    cfg = gol.native.EngineConfig()
    cfg.backend, cfg.rule, cfg.kernel, cfg.device = "hip", HIGHLIFE, "tile", 0
    with pytest.raises(gol.native.GolError) as e:
        gol.native.Engine.create(s.geometry, cfg, s.transport)
    assert "tile" in str(e.value) and HIGHLIFE in str(e.value)


def _thread_ranks(gol, P, N, gens, **kw):
    ts = gol.parallel.p2p_thread_transports(P)
    out, errs = [None] * P, []

    def rank_main(r):
        try:
            s = gol.Simulation(N, ts[r], backend="hip", device=0, global_mode=True, rule=HIGHLIFE, **kw)
            s.init(5, seed=17)
            assert s.stats()["kernel"].startswith("rule@"), s.stats()
            s.step(gens)
            out[r] = (s.geometry.row0, s.geometry.col0, s.board())
        except Exception as e:  # pragma: no cover - reported below
            errs.append(repr(e))

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    ref = numpy_step_rule(initial_board(5, N, 1, True, 17), HIGHLIFE, gens)
    for r0, c0, b in out:
        assert np.array_equal(b, ref[r0 : r0 + b.shape[0], c0 : c0 + b.shape[1]])


@pytest.mark.parametrize("schedule", ["full", "split"])
@pytest.mark.parametrize("P", [2, 3])
def test_thread_ranks_1d(gol, P, schedule):
    _thread_ranks(gol, P, 512, 16 * 4 + 5, halo_depth=16, schedule=schedule)


def test_thread_ranks_2x2(gol):
    _thread_ranks(gol, 4, 512, 16 * 4 + 5, halo_depth=16, decomp="2d", grid="2x2")


@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


@pytest.mark.parametrize("kw", [{"schedule": "split"}, {"schedule": "full"}, {"decomp": "2d"}],
                         ids=["1d-split", "1d-full", "2d"])
def test_rccl_self(gol, rccl, kw):
    """Every halo path of the multi-GPU engine on one rank, under a rule (modelled on test_rccl_self_1d)."""
    N, R = 1024, 8
    gens = 3 * R + 5
    s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=HIGHLIFE, halo_depth=R, subtiles=0, **kw)
    s.init(5, seed=R)
    s.step(gens)
    st = s.stats()
    got = s.board()
    s.synchronize()
    assert st["kernel"].startswith("rule@") and st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
    if "schedule" in kw:
        assert st["schedule"] == kw["schedule"], st
    assert np.array_equal(got, numpy_step_rule(initial_board(5, N, 1, True, R), HIGHLIFE, gens))
