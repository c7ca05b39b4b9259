"""Generations rules on the HIP backend: the kernel step_gen<K, M> (generations_kernel.hip) with k_state_counts and
k_settle_decay (aux_kernels.hip) against the numpy oracle ``numpy_generations``: every pass depth of every plane count,
tail and three-row boards, both boundaries, wide boards with full-width segments, multi-pass supersteps, a stamp
between runs, a hinted run, and the CPU backend.

Every comparison is exact (generations_cases.check: the board, state_counts(), population() and the ``gen@K`` kernel),
and the oracle-only conditions of generations_cases.lively come first: every state occurs at the compared generation,
and with passes of two generations or more some cell is dying strictly inside a pass."""
import numpy as np
import pytest

import generations_cases as gc
import wide_cases as wc
from gol_amd.ops import initial_board, numpy_generations, random_board

pytestmark = pytest.mark.gpu

SWEEP = [(M, K) for M in (1, 2, 3) for K in range(1, gc.KMAX[M] + 1)]
WIDE = [wc.S3968, wc.S3950]  # one aligned (the x-wrap in the plan), one with a tail word (ghost words on the torus)


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


def test_depths_are_instantiated(gol):
    """The depths the sweep runs are the depths the kernels are built for."""
    for M, rule in gc.GPU_RULES.items():
        assert gol.native.max_generations_depth(gc.STATES[rule]) == gc.KMAX[M]
    assert [gol.native.max_generations_depth(c) for c in range(3, 10)] == [8, 5, 5, 2, 2, 2, 2]


@pytest.mark.parametrize("hw", gc.BOARDS, ids=gc.board_id)
@pytest.mark.parametrize("M,K", SWEEP, ids=[f"M{m}-K{k}" for m, k in SWEEP])
def test_sweep(gol, M, K, hw):
    """Every pass depth of every plane count on every size class (tail words of 63, 1 and 9 cells, packed segments in the
    per-lane runner, rows that wrap several times per pass): 2K + 1 generations, a full pass, a second, a remainder."""
    H, W = hw
    kernel = f"gen@{min(K, H)}"  # (a 3-row board clamps the halo depth, and with it the pass, to its rows)
    for boundary in gc.BOUNDARIES:
        gc.run_case(lambda n, **kw: _sim(gol, n, **kw), gc.GPU_RULES[M], H, W, boundary, K, K=K, kernel=kernel)


@pytest.mark.parametrize("shape", WIDE, ids=[wc.shape_id(s) for s in WIDE])
@pytest.mark.parametrize("M,K", [(M, K) for M in (1, 2, 3) for K in (1, gc.KMAX[M])], ids=lambda v: str(v))
def test_wide(gol, M, K, shape):
    """Full-width segments in the scalar runner (wide_cases.py tells what each shape gives)."""
    for boundary in gc.BOUNDARIES:
        gc.run_case(lambda n, **kw: _sim(gol, n, **kw), gc.GPU_RULES[M], shape.H, shape.W, boundary, K, K=K, kernel=f"gen@{K}")


@pytest.mark.parametrize("passes", [2, 3])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_multipass_supersteps(gol, M, passes):
    """Supersteps of two and three passes of the deepest depth: the later passes read the counter of the rows the earlier
    ones stored; launches are eager."""
    K, N = gc.KMAX[M], 200
    R = passes * K
    for boundary in gc.BOUNDARIES:
        s = gc.run_case(lambda n, **kw: _sim(gol, n, **kw), gc.GPU_RULES[M], N, N, boundary, R, K=K, kernel=f"gen@{K}")
        st = s.stats()
        assert st["depth"] == R and st["kernel_depth"] == K and st["graph_launches"] == 0, st


@pytest.mark.parametrize("M", [1, 2, 3])
def test_stamp_between_runs(gol, M):
    """A stamp between two runs: it acts on the live plane and clears the counter of the cells it makes alive
    (k_settle_decay); the oracle applies the same to its states."""
    rule, K, H, W = gc.GPU_RULES[M], gc.KMAX[M], 65, 137
    C, seed = gc.STATES[rule], gc.seed_of(65, 137, gc.GPU_RULES[M], "torus")
    g1, g2 = 2 * K + 1, K + 2
    h = gc.history(H, W, seed, rule, "torus", g1)
    pat = random_board(20, 90, 5)
    s = gc.start_sim(_sim(gol, H, width=W, rule=rule, halo_depth=K, kernel_depth=K), H, W, seed, rule)
    s.step(g1)
    gc.check(s, h[g1], f"gen@{K}")
    s.stamp(pat, at=(55, 100), mode="or")  # across both seams
    live = (h[g1] == 1).astype(np.uint8)
    rr, cc = np.ix_(np.arange(55, 75) % H, np.arange(100, 190) % W)
    live[rr, cc] |= pat
    want = np.where(live == 1, 1, h[g1]).astype(np.uint8)
    assert ((want == 1) & (h[g1] >= 2)).any()  # some stamped cell was dying
    gc.check(s, want)
    ref = numpy_generations(want, rule, g2)
    assert set(np.unique(ref).tolist()) == set(range(C))
    s.step(g2)
    gc.check(s, ref, f"gen@{K}")


@pytest.mark.parametrize("M", [1, 2, 3])
def test_run_hint_prediction_leaves_nothing(gol, M):
    """The init-time timing of a hinted run leaves the board and the decay planes as initialised."""
    rule, N, gens = gc.GPU_RULES[M], 200, 21
    start = initial_board(5, N, 1, True, 3)
    ref = numpy_generations(start, rule, gens)
    assert set(np.unique(ref).tolist()) == set(range(min(gc.STATES[rule], gens + 2)))
    s = _sim(gol, N, rule=rule, halo_depth=8, run_hint=gens).init(5, seed=3)
    assert s.generation == 0
    gc.check(s, start, f"gen@{gc.KMAX[M]}")
    s.step(gens)
    gc.check(s, ref)
    assert s.stats()["graph_launches"] == 0


@pytest.mark.parametrize("M", [1, 2, 3])
def test_cpu_against_hip(gol, M):
    rule, K, N = gc.GPU_RULES[M], gc.KMAX[M], 137
    for boundary in gc.BOUNDARIES:
        seed = gc.seed_of(N, N, rule, boundary)
        sims = [gc.start_sim(gol.Simulation(N, backend=b, device=0, rule=rule, boundary=boundary, halo_depth=8, kernel_depth=K),
                             N, N, seed, rule) for b in ("hip", "cpu")]
        for s in sims:
            s.step(19)
        assert np.array_equal(sims[0].board(), sims[1].board())
        assert sims[0].state_counts().tolist() == sims[1].state_counts().tolist()
        assert sims[0].fingerprint() == sims[1].fingerprint() and sims[0].signature() == sims[1].signature()
        assert set(np.unique(sims[0].board()).tolist()) == set(range(gc.STATES[rule]))
