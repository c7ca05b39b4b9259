"""Larger than Life rules on the HIP backend: the kernel step_ltl<R> (ltl_kernel.hip) against the numpy oracle
``numpy_ltl``: every range with an M1 and an M0 rule, tail-word and all-rows-wrap shapes, both boundaries, wide boards
with full-width segments, B3/S23 through step_ltl<1> against step_rule, a stamp between runs, a hinted run, the CPU
backend, and the tensor and match readers.

Every comparison is exact (ltl_cases.check: the board, population() and the ``ltl@1`` kernel), and the oracle-only
conditions of ltl_cases.preconditions come first: every threshold is exercised from both sides on the start board, each
generation changes the board, and the bounded result differs from the torus result."""
import numpy as np
import pytest

import ltl_cases as lc
import wide_cases as wc
from gol_amd.ops import initial_board, match_template, numpy_ltl, numpy_match, random_board

pytestmark = pytest.mark.gpu

WIDE = [wc.S3968, wc.S3950]  # one aligned (the x-wrap in the plan), one with a tail word (ghost words on the torus)
LIFE_AS_LTL = ["R1,C0,M0,S2..3,B3..3,NM", "R1,C0,M1,S3..4,B3..3,NM"]


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


@pytest.mark.parametrize("boundary", lc.BOUNDARIES)
@pytest.mark.parametrize("R", lc.RANGES)
def test_sweep(gol, R, boundary):
    """Every shape of the range under both rules (tail words of 63, 1 and 9 cells, packed segments in the per-lane
    runner, 2R + 1 rows that every window wraps around): two generations, compared after each."""
    for rule in lc.rules(R):
        for H, W in lc.shapes(R):
            lc.run_case(lambda n, **kw: _sim(gol, n, **kw), rule, H, W, boundary, kernel="ltl@1")


@pytest.mark.parametrize("shape", WIDE, ids=[wc.shape_id(s) for s in WIDE])
@pytest.mark.parametrize("R", lc.WIDE_RANGES)
def test_wide(gol, R, shape):
    """Full-width segments in the scalar runner (wide_cases.py tells what each shape gives)."""
    for rule in lc.rules(R):
        for boundary in lc.BOUNDARIES:
            lc.run_case(lambda n, **kw: _sim(gol, n, **kw), rule, shape.H, shape.W, boundary, kernel="ltl@1")


@pytest.mark.parametrize("rule", LIFE_AS_LTL)
def test_life_through_step_ltl(gol, rule):
    """B3/S23 through step_ltl<1> against step_rule: 17 generations at 137 x 137 on the usual random board."""
    start = random_board(137, 137, 3)
    for boundary in lc.BOUNDARIES:
        a = _sim(gol, 137, rule=rule, boundary=boundary)
        b = _sim(gol, 137, rule="B3/S23", kernel="rule", boundary=boundary)
        for s in (a, b):
            s.init(0)
            s.set_board(start)
            s.step(17)
        assert a.stats()["kernel"] == "ltl@1" and b.stats()["kernel"].startswith("rule@")
        assert np.array_equal(a.board(), b.board()) and a.board().any()
        assert a.signature() == b.signature() and a.population() == b.population()


@pytest.mark.parametrize("R", lc.RANGES)
def test_three_generations(gol, R):
    """Three generations at 137 x 137 in one step() call, where every rule keeps changing."""
    for rule in lc.rules(R):
        for boundary in lc.BOUNDARIES:
            seed = lc.seed_of(137, 137, rule, boundary)
            assert lc.lively(137, 137, seed, rule, boundary, 3)
            h = lc.history(137, 137, seed, rule, boundary, 3)
            s = lc.start_sim(_sim(gol, 137, rule=rule, boundary=boundary), 137, 137, seed)
            s.step(3)
            assert s.generation == 3
            lc.check(s, h[3], "ltl@1")


@pytest.mark.parametrize("R", [1, 5, 7])
def test_stamp_between_runs(gol, R):
    """A stamp between two runs, across both seams of the torus."""
    rule, H, W = lc.rule_m1(R), 65, 137
    seed = lc.seed_of(H, W, rule, "torus")
    b1 = numpy_ltl(lc.start_board(H, W, seed), rule, 2)
    s = lc.start_sim(_sim(gol, H, width=W, rule=rule), H, W, seed)
    s.step(2)
    lc.check(s, b1, "ltl@1")
    pat = random_board(20, 90, 5)
    s.stamp(pat, at=(55, 100), mode="or")
    want = b1.copy()
    rr, cc = np.ix_(np.arange(55, 75) % H, np.arange(100, 190) % W)
    want[rr, cc] |= pat
    assert not np.array_equal(want, b1)
    lc.check(s, want)
    ref = numpy_ltl(want, rule, 3)
    assert not np.array_equal(ref, numpy_ltl(b1, rule, 3)) and 0 < ref.sum() < ref.size
    s.step(3)
    lc.check(s, ref, "ltl@1")


@pytest.mark.parametrize("R", [1, 5, 7])
def test_run_hint_prediction_leaves_nothing(gol, R):
    """The init-time autotune and a hinted run's prediction run on scratch state: the board is as initialised."""
    rule, N, gens = lc.rule_m0(R), 200, 5
    seed = lc.seed_of(N, N, rule, "torus")
    start = lc.start_board(N, N, seed)
    ref = numpy_ltl(start, rule, gens)
    assert not np.array_equal(ref, start) and 0 < ref.sum() < ref.size
    s = _sim(gol, N, rule=rule, run_hint=gens).init(5, seed=3)
    assert s.generation == 0 and np.array_equal(s.board(), initial_board(5, N, 1, True, 3))  # as initialised
    s.set_board(start)
    s.step(gens)
    lc.check(s, ref, "ltl@1")
    assert s.stats()["graph_launches"] == 0


@pytest.mark.parametrize("R", lc.RANGES)
def test_cpu_against_hip(gol, R):
    for rule in lc.rules(R):
        for boundary in lc.BOUNDARIES:
            seed = lc.seed_of(137, 137, rule, boundary)
            sims = [lc.start_sim(gol.Simulation(137, backend=b, device=0, rule=rule, boundary=boundary), 137, 137, seed)
                    for b in ("hip", "cpu")]
            for s in sims:
                s.step(3)
            assert np.array_equal(sims[0].board(), sims[1].board()) and sims[0].board().any()
            assert sims[0].fingerprint() == sims[1].fingerprint() and sims[0].signature() == sims[1].signature()


def test_tensor_and_match_readers(gol):
    """board_tensor() and match() of a small block on an LtL simulation equal those taken from board()."""
    rule, H, W = lc.BOSCO, 65, 137
    seed = lc.seed_of(H, W, rule, "torus")
    s = lc.start_sim(_sim(gol, H, width=W, rule=rule), H, W, seed)
    s.step(2)
    board = s.board()
    lc.check(s, numpy_ltl(lc.start_board(H, W, seed), rule, 2), "ltl@1")
    t = s.board_tensor()
    assert t.is_cuda and np.array_equal(t.cpu().numpy().astype(np.uint8), board)
    block = np.ones((2, 2), np.uint8)
    got = s.match(block, margin=0)
    pos, _ = numpy_match(board, match_template(block, margin=0))
    assert got.count == len(pos) > 0 and np.array_equal(got.positions, pos)
    assert s.count_matches(block, margin=0) == len(pos)
    win = s.window(60, 130, 12, 20)
    assert np.array_equal(win, board[np.ix_(np.arange(60, 72) % H, np.arange(130, 150) % W)])


def test_engine_refuses_the_other_kernels(gol):
    geo = gol.native.make_geometry(gol.native.make_decomposition(64, 1, False, "1d", "", 0), 0)
    for kernel in ("temporal", "tile", "pipe", "resident", "lds"):
        cfg = gol.native.EngineConfig()
        cfg.backend = "hip"
        cfg.rule = lc.BOSCO
        cfg.kernel = kernel
        with pytest.raises(gol.native.GolError, match=kernel) as e:
            gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
        assert lc.BOSCO in str(e.value)
