"""Census mode on the HIP backend: the kernel step_census<K> (census_kernel.hip) under every schedule the rule
kernels run under -- pass depths, board sizes, wrap and ghost rows, both boundaries, multi-pass supersteps, several
step() calls, thread ranks sharing the GPU, the 1-rank RCCL communicator -- against the numpy oracle ``numpy_census``.

Every comparison is exact, and each also asserts that the final board is the oracle's (counting must not disturb
stepping), that the last count is ``population()`` and that the series holds at least two distinct values.  Random
boards keep the ghost rows and the ghost words live, so a count that includes a redundantly computed cell is wrong."""
import functools
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_census, numpy_step_rule, numpy_step_rule_bounded, random_board

pytestmark = pytest.mark.gpu

HIGHLIFE = "B36/S23"
# B1 rules put births just outside a bounded board and into the tail bits of an unaligned last word
RULES = ["B3/S23", HIGHLIFE, "B1357/S1357", "B1/S012345678"]
BOUNDARIES = ["torus", "dead"]
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8]


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    kw.setdefault("census", True)
    return gol.Simulation(N, **kw)


@functools.lru_cache(maxsize=None)
def sweep_reference(N, rule, boundary):
    """The oracle's series of the sweep's N x N board (seed N) over the longest run, 17 generations, and the boards
    after every odd generation: computed once per (N, rule, boundary) and shared by the depths."""
    b = initial_board(5, N, 1, True, N)
    counts, boards = [], {}
    for g in range(1, 2 * max(DEPTHS) + 2):
        b = (numpy_step_rule_bounded if boundary == "dead" else numpy_step_rule)(b, rule, 1)
        counts.append(int(b.sum()))
        if g % 2:
            boards[g] = b
    return np.array(counts, np.uint64), boards


@functools.lru_cache(maxsize=None)
def reference(N, seed, rule, boundary, gens):
    return numpy_census(initial_board(5, N, 1, True, seed), rule, gens, bounded=boundary == "dead", return_board=True)


def check(sim, start, counts, board, tiny=False):
    got_start, got = sim.census()
    assert got_start == start and got.dtype == np.uint64
    assert np.array_equal(got, counts), (got.tolist(), np.asarray(counts).tolist())
    assert np.array_equal(sim.board(), board)
    assert int(got[-1]) == sim.population()
    assert tiny or len(set(got.tolist())) >= 2


def test_depths_are_instantiated(gol):
    assert gol.native.max_census_depth() == max(DEPTHS) >= 4


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000])
@pytest.mark.parametrize("K", DEPTHS)
def test_sweep(gol, K, N):
    """Every pass depth on every size class (ROWS_WRAP on boards shorter than the pass, unaligned widths, packed narrow
    segments, several blocks): 2K + 1 generations, a full superstep and the remainders."""
    gens = 2 * K + 1
    for boundary in BOUNDARIES:
        for rule in RULES:
            counts, boards = sweep_reference(N, rule, boundary)
            s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K).init(5, seed=N)
            st = s.stats()
            assert st["kernel"].startswith("census@") and st["census"] is True and st["boundary"] == boundary, st
            s.step(gens)
            assert s.stats()["graph_launches"] == 0
            check(s, 0, counts[:gens], boards[gens], tiny=N <= 3)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("H,W", [(70, 130), (100, 200), (200, 64), (5, 1000)])
def test_rectangular(gol, H, W, boundary):
    """Unaligned tails, an aligned one-word board, and a strip shorter than the pass depth."""
    gens = 17
    for rule in (HIGHLIFE, "B1/S012345678"):
        counts, board = numpy_census(random_board(H, W, 5), rule, gens, bounded=boundary == "dead", return_board=True)
        s = _sim(gol, H, rule=rule, boundary=boundary, width=W, halo_depth=8).init(5, seed=5)
        assert s.stats()["kernel"].startswith("census@"), s.stats()
        s.step(gens)
        check(s, 0, counts, board)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("passes", [2, 3])
@pytest.mark.parametrize("N", [137, 1000])
def test_multipass_supersteps(gol, N, passes, boundary):
    """Supersteps of two and three passes of the deepest depth: the extension rows the earlier passes compute beyond
    the tile are not counted."""
    D = gol.native.max_census_depth()
    R, gens = passes * D, 37
    for rule in (HIGHLIFE, "B1/S012345678"):
        s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=R, kernel_depth=D).init(5, seed=6)
        st = s.stats()
        assert st["depth"] == R and st["kernel_depth"] == D and st["kernel"].startswith(f"census@{D}"), st
        s.step(gens)
        counts, board = reference(N, 6, rule, boundary, gens)
        check(s, 0, counts, board)


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_several_steps_stamp_init_restore(gol, tmp_path, boundary):
    """One continuous series over several step() calls and a stamp(); init() and restore() clear it and set start."""
    N, rule, bounded = 137, HIGHLIFE, boundary == "dead"
    s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=8).init(5, seed=8)
    assert s.census()[0] == 0 and len(s.census()[1]) == 0  # (the init-time timing launches left nothing)
    b = initial_board(5, N, 1, True, 8)
    s.step(5).step(20).step(1)
    c1, b = numpy_census(b, rule, 26, bounded=bounded, return_board=True)
    check(s, 0, c1, b)
    s.stamp(np.ones((3, 3), np.uint8), at=(3, 3), mode="xor")  # the generation count runs on: so does the series
    b = s.board()
    s.step(7)
    c2, b = numpy_census(b, rule, 7, bounded=bounded, return_board=True)
    check(s, 0, np.concatenate([c1, c2]), b)
    s.checkpoint(str(tmp_path / "c"))
    s.census_clear()
    assert s.census()[0] == 33 and len(s.census()[1]) == 0
    s.step(3)
    c3, b3 = numpy_census(b, rule, 3, bounded=bounded, return_board=True)
    check(s, 33, c3, b3)
    s.init(5, seed=8)
    assert s.census()[0] == 0 and len(s.census()[1]) == 0
    s.step(2)
    assert np.array_equal(s.census()[1], c1[:2])
    assert s.restore(str(tmp_path / "c")) == 33
    assert s.census()[0] == 33 and len(s.census()[1]) == 0
    s.step(3)
    check(s, 33, c3, b3)


def test_run_hint_prediction_leaves_no_record(gol):
    """A hinted simulation times whole runs on the live board at init (and restores it): none of it is recorded."""
    N, gens = 200, 20
    s = _sim(gol, N, rule=HIGHLIFE, halo_depth=8, run_hint=gens).init(5, seed=3)
    assert s.generation == 0 and len(s.census()[1]) == 0
    s.step(gens)
    counts, board = reference(N, 3, HIGHLIFE, "torus", gens)
    check(s, 0, counts, board)


def _thread_ranks(gol, P, N, gens, rule, boundary, global_mode, **kw):
    """P ranks as threads on one GPU (p2p emulation), then on the CPU backend: per backend the global board and every
    rank's (start, series, population)."""
    out = {}
    for backend in ("hip", "cpu"):
        ts = gol.parallel.p2p_thread_transports(P) if backend == "hip" else gol.parallel.thread_transports(P)
        parts, errs = [None] * P, []

        def rank_main(r):
            try:
                skw = dict(kw, device=0) if backend == "hip" else {k: v for k, v in kw.items() if k != "schedule"}
                s = gol.Simulation(N, ts[r], backend=backend, global_mode=global_mode, rule=rule, boundary=boundary,
                                   census=True, **skw)
                s.init(5, seed=17)
                if backend == "hip":
                    st = s.stats()
                    assert st["kernel"].startswith("census@"), st
                    if "schedule" in kw:
                        assert st["schedule"] == kw["schedule"], st
                        assert ("+boundary:census@" in st["kernel"]) == (kw["schedule"] == "split"), st
                s.step(gens)
                start, counts = s.census()
                parts[r] = (s.geometry.row0, s.geometry.col0, s.board(), start, counts, s.population())
            except Exception as e:  # pragma: no cover - reported below
                errs.append(repr(e))

        th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs
        H = max(r0 + b.shape[0] for r0, _, b, *_ in parts)
        W = max(c0 + b.shape[1] for _, c0, b, *_ in parts)
        full = np.zeros((H, W), np.uint8)
        for r0, c0, b, *_ in parts:
            full[r0 : r0 + b.shape[0], c0 : c0 + b.shape[1]] = b
        out[backend] = (full, parts)
    return out


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("kw", [{"schedule": "split"}, {"schedule": "full"}, {"decomp": "2d", "grid": "2x2"}],
                         ids=["P4-split", "P4-full", "2x2"])
def test_thread_ranks(gol, kw, boundary):
    """Four ranks of 200 x 200 cells, as strips or as a 2 x 2 grid; supersteps of two passes, so the earlier pass
    stores ghost rows (in the grid ghost words too), and a one-pass remainder.  Every rank gets the same, global
    series, on both backends."""
    P, gens, two_d = 4, 40, "grid" in kw
    start_board = initial_board(5, 400, 1, True, 17) if two_d else initial_board(5, 200, P, True, 17)
    for rule in (HIGHLIFE, "B1/S012345678"):
        counts, board = numpy_census(start_board, rule, gens, bounded=boundary == "dead", return_board=True)
        got = _thread_ranks(gol, P, 400 if two_d else 200, gens, rule, boundary, two_d, halo_depth=16, kernel_depth=8, **kw)
        for backend in ("hip", "cpu"):
            full, parts = got[backend]
            assert np.array_equal(full, board), (backend, rule)
            for _, _, _, start, series, pop in parts:
                assert start == 0 and np.array_equal(series, counts), (backend, rule)
                assert pop == int(counts[-1])
        assert len(set(counts.tolist())) >= 2


@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("kw", [{}, {"decomp": "2d"}], ids=["1d", "2d"])
def test_rccl_self(gol, rccl, kw, boundary):
    """Every halo path of the multi-GPU engine on one rank: the rank is its own neighbour through the transport, so
    its ghost rows (and, 2-D, ghost words) are stored by exchanges and by the earlier passes of a superstep."""
    N, R, gens = 256, 16, 40
    for rule in (HIGHLIFE, "B1/S012345678"):
        s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=rule, boundary=boundary, halo_depth=R,
                           kernel_depth=8, subtiles=0, census=True, **kw)
        s.init(5, seed=R)
        s.step(gens)
        st = s.stats()
        assert st["kernel"].startswith("census@") and st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
        counts, board = reference(N, R, rule, boundary, gens)
        check(s, 0, counts, board)
        s.synchronize()


def test_refusals(gol):
    D = gol.native.max_census_depth()
    for kw, word in [({"compat": True}, "compat"), ({"subtiles": 2}, "subtiles=2"), ({"kernel_depth": D + 1}, f"{D} generations")]:
        with pytest.raises(ValueError) as e:
            _sim(gol, 64, **kw)
        assert word in str(e.value)
    sim = _sim(gol, 64)
    for kernel in ("temporal", "tile", "pipe", "resident", "lds"):
        with pytest.raises(ValueError) as e:
            _sim(gol, 64, kernel=kernel)
        assert "counts no census" in str(e.value)
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.census, cfg.kernel, cfg.device = "hip", True, kernel, 0
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(sim.geometry, cfg, sim.transport)
        assert f"kernel '{kernel}' counts no census" in str(e.value)
    # the native engine on its own: compat, sub-tiles, a pass deeper than the census kernel's
    for field, value, word in [("compat", True, "census"), ("subtiles", 2, "census"), ("kernel_depth", D + 1, f"{D} generations")]:
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.census, cfg.device = "hip", True, 0
        setattr(cfg, field, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(sim.geometry, cfg, sim.transport)
        assert word in str(e.value)


def test_stats_and_non_census(gol):
    s = _sim(gol, 256, halo_depth=8).init(5, seed=1)  # B3/S23 on the torus: the census kernel all the same
    st = s.stats()
    assert st["kernel"].startswith("census@") and st["census"] is True and st["rule"] == "B3/S23", st
    s.step(9)
    counts, board = reference(256, 1, "B3/S23", "torus", 9)
    check(s, 0, counts, board)
    plain = _sim(gol, 256, census=False, halo_depth=8).init(5, seed=1)
    assert plain.stats()["census"] is False and not plain.stats()["kernel"].startswith("census@")
    with pytest.raises(ValueError):
        plain.census()
    with pytest.raises(gol.native.GolError):
        plain.engine.census()
