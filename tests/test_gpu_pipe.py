"""step_pipe (csrc/src/hip/pipe_kernel.hip): level-pipelined workgroups, one loader wave and NW - 1
stages of L generations chained through LDS rings.  Boards after G generations against numpy (small
boards), a PyTorch fp32 conv2d torus step on cuda:0 (large ones) and the thread-rank transport (ghost
rows from neighbours).  Rule: gol-with-cuda.cu:239-257.

The tests that name a geometry have a ``_pinned`` twin.  Unpinned, as production does: the engine measures
step_temporal and the step_pipe geometries per depth and cuts the supersteps from the cheapest, so which kernel runs is
the measurement's choice; the ``cut`` entries of stats()["tuning"] say which, and are printed.  Pinned: kernel_depth = K
keeps the engine from measuring, every pass of K generations is step_pipe in the named geometry, and the ``cut`` entry
is asserted.  test_gpu_pipe_geometries.py runs all 48 instantiations pinned."""
import functools
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_step, random_board, torch_step

pytestmark = pytest.mark.gpu


def _sim(gol, N, geo, monkeypatch, **kw):
    monkeypatch.setenv("GOL_PIPE", geo)
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    kw.setdefault("kernel", "pipe")
    return gol.Simulation(N, **kw)


@functools.lru_cache(maxsize=None)
def _after(N, seed, gens):
    """The numpy board of a test and its pinned twin, computed once."""
    b = numpy_step(initial_board(5, N, 1, True, seed), gens)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _rectangular_refs(N, W, seed, steps):
    out, ref = [], random_board(N, W, seed)
    for g in steps:
        ref = numpy_step(ref, g)
        ref.setflags(write=False)
        out.append(ref)
    return out


def _geometry(geo):
    nw, L, wg = (int(x) for x in geo.split(","))
    return nw, L, wg, (nw - 1) * L


def _pin(geo, halo_depth=None):
    """The arguments that pin every pass of K generations to step_pipe in geometry ``geo``."""
    K = _geometry(geo)[3]
    return dict(kernel_depth=K, halo_depth=K if halo_depth is None else halo_depth, subtiles=0)


def _cuts(stats):
    return [t for t in stats["tuning"].split() if t.startswith("cut")]


def _check_cut(stats, geo, R, pinned, what):
    """Pinned: supersteps of R generations are whole step_pipe passes in geometry ``geo`` and a step_temporal pass of
    the rest.  Unpinned: the measured cut is printed, not asserted."""
    nw, L, wg, K = _geometry(geo)
    if not pinned:
        print(f"unpinned {what}: kernel {stats['kernel']}, depth {stats['depth']}, {' '.join(_cuts(stats))}")
        return
    one = f"pipe@{K}({nw - 1}x{L},{wg}/CU)"
    assert stats["kernel"] == one and stats["kernel_depth"] == K and stats["depth"] == R, stats
    want = f"cut{R}=" + "+".join([one] * (R // K) + ([f"temporal@{R % K}"] if R % K else []))
    assert want in stats["tuning"].split(), (want, stats["tuning"])


VS_NUMPY = [(64, 1, "9,3,2"), (64, 29, "9,3,2"), (256, 40, "9,3,2"), (512, 77, "13,2,1"),
            (640, 100, "9,2,2"), (1024, 50, "5,4,4"), (1024, 61, "7,3,2"),
            (2048, 45, "11,2,2"), (512, 33, "16,2,1"), (768, 48, "5,1,1")]


def _vs_numpy(gol, monkeypatch, N, gens, geo, pinned):
    nw, L, _, K = _geometry(geo)
    s = _sim(gol, N, geo, monkeypatch, **(_pin(geo) if pinned else {})).init(5, seed=N + gens)
    assert s.stats()["kernel"].startswith(f"pipe@{(nw - 1) * L}"), s.stats()
    _check_cut(s.stats(), geo, K, pinned, f"test_pipe_vs_numpy {N} {gens} {geo}")
    s.step(gens)
    assert np.array_equal(s.board(), _after(N, N + gens, gens))


@pytest.mark.parametrize("N,gens,geo", VS_NUMPY)
def test_pipe_vs_numpy(gol, monkeypatch, N, gens, geo):
    _vs_numpy(gol, monkeypatch, N, gens, geo, False)


@pytest.mark.parametrize("N,gens,geo", VS_NUMPY)
def test_pipe_vs_numpy_pinned(gol, monkeypatch, N, gens, geo):
    _vs_numpy(gol, monkeypatch, N, gens, geo, True)


def _rectangular_and_repeated(gol, monkeypatch, pinned):
    N, W, geo = 300, 1024, "9,3,2"
    s = _sim(gol, N, geo, monkeypatch, width=W, **(_pin(geo) if pinned else {})).init(5, seed=3)
    _check_cut(s.stats(), geo, 24, pinned, "test_pipe_rectangular_and_repeated")
    steps = (24, 5, 48, 1, 30)
    for g, ref in zip(steps, _rectangular_refs(N, W, 3, steps)):
        s.step(g)
        assert np.array_equal(s.board(), ref), g


def test_pipe_rectangular_and_repeated(gol, monkeypatch):
    _rectangular_and_repeated(gol, monkeypatch, False)


def test_pipe_rectangular_and_repeated_pinned(gol, monkeypatch):
    _rectangular_and_repeated(gol, monkeypatch, True)


def test_pipe_8192_vs_torch(gol, monkeypatch):
    import torch

    N, seed = 8192, 0x5EED
    s = _sim(gol, N, "9,3,2", monkeypatch, run_hint=1000).init(5, seed=seed)
    ref = torch.as_tensor(initial_board(5, N, 1, True, seed), device="cuda:0")
    for g in (100, 37):
        s.step(g)
        ref = torch_step(ref, g, device="cuda:0")
        got = s.board()
        assert np.array_equal(got, ref.cpu().numpy()), f"{int((got != ref.cpu().numpy()).sum())} cells differ"


RANKS = [(2, 32), (3, 32), (2, 128)]


def _thread_ranks_ghost_rows(gol, monkeypatch, P, R, pinned):
    """Ranks with neighbours: the loader reads the exchanged ghost rows (no wrap); a superstep of R
    generations runs as 24-deep step_pipe passes (the earlier ones also computing the ghost rows the
    later ones read) plus step_temporal passes for the rest."""
    N = 384 if R == 32 else 768
    gens = R * 3 + 11
    geo = "9,3,2"
    monkeypatch.setenv("GOL_PIPE", geo)
    ts = gol.parallel.p2p_thread_transports(P)
    out, errs, stats = [None] * P, [], [None] * P
    kw = dict(kernel_depth=24) if pinned else {}

    def rank_main(r):
        try:
            s = gol.Simulation(N, ts[r], backend="hip", device=0, global_mode=True, halo_depth=R, kernel="pipe",
                               overlap=False, subtiles=0, **kw)
            s.init(5, seed=21)
            stats[r] = s.stats()
            s.step(gens)
            out[r] = (s.geometry.row0, s.board())
        except Exception as e:  # pragma: no cover - reported below
            errs.append(repr(e))

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    for r in range(P):
        _check_cut(stats[r], geo, R, pinned, f"test_pipe_thread_ranks_ghost_rows P={P} R={R} rank {r}")
    board = np.zeros((N, N), dtype=np.uint8)
    for r0, b in out:
        board[r0 : r0 + b.shape[0]] = b
    assert np.array_equal(board, _after(N, 21, gens))


@pytest.mark.parametrize("P,R", RANKS)
def test_pipe_thread_ranks_ghost_rows(gol, monkeypatch, P, R):
    _thread_ranks_ghost_rows(gol, monkeypatch, P, R, False)


@pytest.mark.parametrize("P,R", RANKS)
def test_pipe_thread_ranks_ghost_rows_pinned(gol, monkeypatch, P, R):
    """kernel_depth = 24: five (R = 128) or one (R = 32) step_pipe passes and a step_temporal pass of 8, asserted."""
    _thread_ranks_ghost_rows(gol, monkeypatch, P, R, True)


def test_pipe_rejects_bad_geometry(gol, monkeypatch):
    with pytest.raises(Exception, match="GOL_PIPE"):
        _sim(gol, 256, "6,2,1", monkeypatch).init(5, seed=1)
    with pytest.raises(Exception, match="halo depth"):
        _sim(gol, 256, "16,4,1", monkeypatch).init(5, seed=1)
