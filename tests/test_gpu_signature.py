"""Signature mode on the HIP backend: the kernel step_signature<K> (signature_kernel.hip) under every schedule the
census kernel runs under -- pass depths, board sizes, wrap and ghost rows, both boundaries, wide boards with full-width
segments, multi-pass supersteps, thread ranks sharing the GPU, rank grids, the 1-rank RCCL communicator -- and
k_signature, k_board_diff and find_cycle(), against the numpy oracles ``numpy_signature`` / ``numpy_census``.

Every comparison is exact, and each also asserts the ``sig@`` kernel, that the final board is the oracle's, that the
populations are ``numpy_census``'s, that the last signature is ``signature()`` and that the series holds at least two
distinct signatures.  Random boards keep the ghost rows and words live, so a hash that includes a redundantly computed
cell is wrong."""
import functools
import threading

import numpy as np
import pytest

import grid_cases as gc
import wide_cases as wc
from cycle_cases import CYCLE_CASES, GRID_CASES, check_cycle, cycle_oracle
from gol_amd.ops import Cycle, numpy_signature, numpy_step_rule, numpy_step_rule_bounded, random_board

pytestmark = pytest.mark.gpu

HIGHLIFE = "B36/S23"
RULES = ["B3/S23", HIGHLIFE, "B1357/S1357", "B1/S012345678"]
BOUNDARIES = ["torus", "dead"]


def depths(gol):
    return list(range(1, gol.native.max_signature_depth() + 1))


MAX_DEPTHS = list(range(1, 9))  # parametrised depths; those above max_signature_depth() have nothing to run


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    kw.setdefault("signature", True)
    return gol.Simulation(N, **kw)


@functools.lru_cache(maxsize=None)
def series(H, W, seed, rule, boundary, gens):
    """The oracle's signatures and populations of generations 1 .. gens of the H x W board of ``seed``, and the boards
    after every odd generation and the last: one numpy generation at a time, computed once and left read-only."""
    step = numpy_step_rule_bounded if boundary == "dead" else numpy_step_rule
    b = random_board(H, W, seed)
    sigs, pops, boards = [], [], {}
    for g in range(1, gens + 1):
        b = step(b, rule, 1)
        sigs.append(numpy_signature(b))
        pops.append(int(b.sum()))
        if g % 2 or g == gens:
            b.setflags(write=False)
            boards[g] = b
    return np.array(sigs, np.uint64), np.array(pops, np.uint64), boards


def check(sim, start, sigs, pops, board, tiny=False):
    got_start, got, got_pops = sim.signatures()
    assert got_start == start and got.dtype == np.uint64 and got_pops.dtype == np.uint64
    assert np.array_equal(sim.board(), board)
    assert np.array_equal(got_pops, pops), (got_pops.tolist(), np.asarray(pops).tolist())
    assert np.array_equal(got, sigs), ([hex(v) for v in got.tolist()], [hex(v) for v in np.asarray(sigs).tolist()])
    assert int(got[-1]) == sim.signature()
    assert int(got_pops[-1]) == sim.population()
    assert tiny or len(set(got.tolist())) >= 2


def test_depths_are_instantiated(gol):
    assert 4 <= gol.native.max_signature_depth() <= 8


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000])
@pytest.mark.parametrize("K", MAX_DEPTHS)
def test_sweep(gol, K, N):
    """Every pass depth on every size class (wrap rows on boards shorter than the pass, where one owned row is computed
    many times; tail words of 1, 63 and 9 cells; packed segments in the per-lane runner; several blocks): 2K + 1
    generations, a full superstep and the remainders."""
    if K > gol.native.max_signature_depth():
        return
    gens, total = 2 * K + 1, 2 * gol.native.max_signature_depth() + 1
    for boundary in BOUNDARIES:
        for rule in RULES:
            sigs, pops, boards = series(N, N, N, rule, boundary, total)
            s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K).init(5, seed=N)
            st = s.stats()
            assert st["kernel"].startswith("sig@") and st["signature"] is True and st["boundary"] == boundary, st
            s.step(gens)
            assert s.stats()["graph_launches"] == 0
            check(s, 0, sigs[:gens], pops[:gens], boards[gens], tiny=N <= 3)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("H,W", [(70, 130), (100, 200), (200, 64), (5, 1000)])
def test_rectangular(gol, H, W, boundary):
    gens = 17
    for rule in (HIGHLIFE, "B1/S012345678"):
        sigs, pops, boards = series(H, W, 5, rule, boundary, gens)
        s = _sim(gol, H, rule=rule, boundary=boundary, width=W, halo_depth=8).init(5, seed=5)
        assert s.stats()["kernel"].startswith("sig@"), s.stats()
        s.step(gens)
        check(s, 0, sigs, pops, boards[gens])


WIDE = [(wc.S3968, 0), (wc.S3950, 0), (wc.S8000, 0), (wc.tail_shape(41), wc.tail_rows(41))]


@pytest.mark.parametrize("shape,rows", WIDE, ids=[wc.shape_id(s) for s, _ in WIDE])
@pytest.mark.parametrize("K", MAX_DEPTHS)
def test_wide(gol, K, shape, rows):
    """Full-width segments in the scalar runner: 64 x 3968 (every band one 64-lane segment, halo lanes 0 / 63),
    64 x 3950 (the tail word is lane 62), 48 x 8000 (a seam between full-width segments, global word index >= 62) and
    two bands of 21 / 20 rows at 4096 columns (row0 > 0 in the scalar runner: the row keys of a band that does not
    start at the tile's first row)."""
    if K > gol.native.max_signature_depth():
        return
    gens = 2 * K + 1
    for boundary in BOUNDARIES:
        for rule in wc.RULES[boundary]:
            sigs, pops, boards = series(shape.H, shape.W, wc.SEED, rule, boundary, wc.SWEEP_GENS)
            s = _sim(gol, shape.H, width=shape.W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K,
                     rows_per_wave=rows).init(5, seed=wc.SEED)
            assert s.stats()["kernel"].startswith("sig@"), s.stats()
            s.step(gens)
            check(s, 0, sigs[:gens], pops[:gens], boards[gens])


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("passes", [2, 3])
@pytest.mark.parametrize("N", [137, 1000])
def test_multipass_supersteps(gol, N, passes, boundary):
    """Supersteps of two and three passes of the deepest depth: the extension rows the earlier passes compute beyond
    the tile are not hashed."""
    D = gol.native.max_signature_depth()
    R, gens = passes * D, 37
    for rule in (HIGHLIFE, "B1/S012345678"):
        s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=R, kernel_depth=D).init(5, seed=6)
        st = s.stats()
        assert st["depth"] == R and st["kernel_depth"] == D and st["kernel"].startswith(f"sig@{D}"), st
        s.step(gens)
        sigs, pops, boards = series(N, N, 6, rule, boundary, gens)
        check(s, 0, sigs, pops, boards[gens])


def test_several_steps_and_clear(gol):
    N, rule = 137, HIGHLIFE
    s = _sim(gol, N, rule=rule, halo_depth=8).init(5, seed=8)
    assert s.signatures()[0] == 0 and len(s.signatures()[1]) == 0  # (the init-time timing launches left nothing)
    s.step(5).step(20).step(1)
    sigs, pops, boards = series(N, N, 8, rule, "torus", 29)
    got = s.signatures()
    assert got[0] == 0 and np.array_equal(got[1], sigs[:26]) and np.array_equal(got[2], pops[:26])
    s.signatures_clear()
    assert s.signatures()[0] == 26 and len(s.signatures()[1]) == 0
    s.step(3)
    check(s, 26, sigs[26:], pops[26:], boards[29])


def test_run_hint_prediction_leaves_no_record(gol):
    N, gens = 200, 21
    s = _sim(gol, N, rule=HIGHLIFE, halo_depth=8, run_hint=gens).init(5, seed=3)
    assert s.generation == 0 and len(s.signatures()[1]) == 0
    s.step(gens)
    sigs, pops, boards = series(N, N, 3, HIGHLIFE, "torus", gens)
    check(s, 0, sigs, pops, boards[gens])


def sig_script(gens):
    def script(s):
        s.step(gens)
        start, sigs, pops = s.signatures()
        return start, sigs, pops, s.signature(), s.population()

    return script


def check_parts(parts, sigs, pops):
    for p in parts:
        start, got, got_pops, sig, pop = p.result
        assert start == 0 and np.array_equal(got, sigs) and np.array_equal(got_pops, pops), p.rank
        assert sig == int(sigs[-1]) and pop == int(pops[-1]), p.rank
    assert len(set(sigs.tolist())) >= 2


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("kw", [{"schedule": "split"}, {"schedule": "full"}, {"decomp": "2d", "grid": "2x2"}],
                         ids=["P4-split", "P4-full", "2x2"])
def test_thread_ranks(gol, kw, boundary):
    """Four thread ranks on hip and on cpu against numpy: strips under the split and the full schedule, and a 2 x 2
    grid, where gword0 > 0.  Supersteps of two passes and a one-pass remainder."""
    H, W = (400, 400) if "grid" in kw else (800, 200)
    rule = HIGHLIFE
    sigs, pops, boards = series(H, W, wc.SEED, rule, boundary, wc.RANK_GENS)
    for backend in ("hip", "cpu"):
        parts = wc.run_ranks(gol, 4, H, W, backend, script=sig_script(wc.RANK_GENS), rule=rule, boundary=boundary,
                             signature=True, **kw)
        if backend == "hip":
            for p in parts:
                assert p.stats["kernel"].startswith("sig@"), p.stats
                if "schedule" in kw:
                    assert ("+boundary:sig@" in p.stats["kernel"]) == (kw["schedule"] == "split"), p.stats
        assert np.array_equal(wc.assemble(H, W, parts), boards[wc.RANK_GENS]), backend
        check_parts(parts, sigs, pops)


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_grid_3x3(gol, boundary):
    """A 3 x 3 grid with a centre rank and tiles of different nw (200 x 448: 192 / 128 / 128 columns)."""
    case = gc.CASES[0]
    sigs, pops, boards = series(case.H, case.W, gc.SEED, HIGHLIFE, boundary, gc.GENS)
    parts = gc.run_ranks(gol, case, "hip", script=sig_script(gc.GENS), rule=HIGHLIFE, boundary=boundary, signature=True)
    assert all(p.stats["kernel"].startswith("sig@") for p in parts)
    gc.check_board(case, parts, boards[gc.GENS])
    check_parts(parts, sigs, pops)


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
    N, R, gens = 256, 16, 40
    s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=HIGHLIFE, boundary=boundary, halo_depth=R,
                       kernel_depth=8 if gol.native.max_signature_depth() >= 8 else 4, subtiles=0, signature=True, **kw)
    s.init(5, seed=R)
    s.step(gens)
    st = s.stats()
    assert st["kernel"].startswith("sig@") and st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
    sigs, pops, boards = series(N, N, R, HIGHLIFE, boundary, gens)
    check(s, 0, sigs, pops, boards[gens])
    s.synchronize()


@pytest.mark.parametrize("kernel", ["temporal", "tile"])
@pytest.mark.parametrize("N", [65, 137, 1000])
def test_signature_of_the_board_in_memory(gol, N, kernel):
    """k_signature: signature() without signature mode, under the B3/S23 kernels."""
    s = _sim(gol, N, signature=False, kernel=kernel, halo_depth=8).init(5, seed=N)
    assert s.signature() == numpy_signature(random_board(N, N, N))
    s.step(9)
    assert not s.stats()["kernel"].startswith("sig@")
    assert s.signature() == int(series(N, N, N, "B3/S23", "torus", 9)[0][-1])
    with pytest.raises(ValueError):
        s.signatures()


def test_snapshot_diff(gol):
    """k_board_diff: 0 right after snapshot(); 9 after a 3 x 3 xor stamp; 1 after a one-cell stamp in the masked tail
    word of a 65-column board."""
    s = _sim(gol, 65, signature=False, halo_depth=8).init(5, seed=3)
    with pytest.raises(gol.native.GolError):
        s.snapshot_diff()
    s.snapshot()
    assert s.snapshot_diff() == 0
    s.stamp(np.ones((3, 3), np.uint8), at=(10, 20), mode="xor")
    assert s.snapshot_diff() == 9
    s.snapshot()
    assert s.snapshot_diff() == 0
    s.stamp(np.ones((1, 1), np.uint8), at=(5, 64), mode="xor")
    assert s.snapshot_diff() == 1
    before = s.board()
    s.step(3)  # (the snapshot is a buffer of its own: stepping does not touch it)
    snap = before.copy()
    snap[5, 64] ^= 1  # the board the snapshot holds: the one before the last stamp
    assert s.snapshot_diff() == int((numpy_step_rule(before, "B3/S23", 3) != snap).sum()) > 1


@pytest.mark.parametrize("name", list(CYCLE_CASES))
def test_find_cycle(gol, name):
    """One rank; the chunks are not multiples of the period, and blinker-8's (3) is below the pass depth."""
    board, rule, boundary, max_generations, chunk = CYCLE_CASES[name]
    H, W = board.shape
    s = _sim(gol, H, width=W, rule=rule, boundary=boundary, halo_depth=8).init(0)
    s.set_board(board)
    assert s.stats()["kernel"].startswith("sig@")
    got = s.find_cycle(max_generations, chunk=chunk)
    want = check_cycle(s, name, got)
    assert np.array_equal(s.board(), want)


def test_find_cycle_budget_ends_first(gol):
    board = CYCLE_CASES["rpent-64"][0]
    s = _sim(gol, 64, halo_depth=8).init(0)
    s.set_board(board)
    assert s.find_cycle(100, chunk=32) is None
    assert s.generation == 100 and np.array_equal(s.board(), numpy_step_rule(board, "B3/S23", 100))


@pytest.mark.parametrize("name", GRID_CASES)
def test_find_cycle_2x2(gol, name):
    board, rule, boundary, max_generations, chunk = CYCLE_CASES[name]
    H, W = board.shape
    P = 4
    ts = gol.parallel.p2p_thread_transports(P)
    out, errs = [None] * P, []

    def worker(r):
        try:
            s = gol.Simulation(H, ts[r], backend="hip", device=0, global_mode=True, width=W, decomp="2d", grid="2x2",
                               halo_depth=8, rule=rule, boundary=boundary, signature=True).init(0)
            s.stamp(board, at=(0, 0), mode="or")
            out[r] = s.find_cycle(max_generations, chunk=chunk)
        except Exception as e:
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not errs, errs
    transient, period, _ = cycle_oracle(name)
    assert all(isinstance(o, Cycle) and o == out[0] for o in out)
    assert (out[0].transient, out[0].period) == (transient, period)


def test_refusals_and_stats(gol):
    D = gol.native.max_signature_depth()
    for kw, word in [({"compat": True}, "compat"), ({"subtiles": 2}, "subtiles=2"), ({"census": True}, "census"),
                     ({"kernel_depth": D + 1}, f"{D} generations")]:
        with pytest.raises(ValueError) as e:
            _sim(gol, 64, **kw)
        assert word in str(e.value)
    sim = _sim(gol, 64)
    for kernel in ("temporal", "tile", "pipe", "resident", "lds"):
        with pytest.raises(ValueError) as e:
            _sim(gol, 64, kernel=kernel)
        assert "records no signatures" in str(e.value)
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.signature, cfg.kernel, cfg.device = "hip", True, kernel, 0
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(sim.geometry, cfg, sim.transport)
        assert f"kernel '{kernel}' records no signatures" in str(e.value)
    for field, value, word in [("compat", True, "signature"), ("subtiles", 2, "signature"), ("census", True, "signature"),
                               ("kernel_depth", D + 1, f"{D} generations")]:
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.signature, cfg.device = "hip", True, 0
        setattr(cfg, field, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(sim.geometry, cfg, sim.transport)
        assert word in str(e.value)
    s = _sim(gol, 256, halo_depth=8).init(5, seed=1)  # B3/S23 on the torus: the signature kernel all the same
    st = s.stats()
    assert st["kernel"].startswith("sig@") and st["signature"] is True and st["census"] is False and st["rule"] == "B3/S23", st
    plain = _sim(gol, 256, signature=False, halo_depth=8).init(5, seed=1)
    assert plain.stats()["signature"] is False and not plain.stats()["kernel"].startswith("sig@")
    with pytest.raises(gol.native.GolError):
        plain.engine.signatures()
