"""Shared by test_generations.py (CPU backend) and test_gpu_generations.py (MI355X): the cases of the Generations rules
(B/S/C), their numpy references (``numpy_generations``, computed once per board, rule and boundary, kept read-only) and
the checks.

Every comparison is exact: ``board()`` against the oracle's state array, ``state_counts()`` against its ``bincount``,
``population()`` against its count of state 1.  Before a backend is compared the oracle alone is asked (``lively``): at
the compared generation every state 0 .. C-1 occurs on its board, and with passes of K >= 2 generations some cell is
dying at a generation strictly inside a pass, so a kernel that dropped the decay counter between its levels could not
pass.  The cases start from a board of random states (``set_board``): a board of live cells alone holds no state above
g + 1 after g generations, and the shallow sweeps compare after three.
"""
import functools

import numpy as np

from gol_amd.ops import numpy_generations

BRAIN, STARWARS, FROGS, C5, C9 = "B2/S/C3", "B2/S345/C4", "B34/S12/C3", "B2/S345/C5", "B2/S345/C9"
STATES = {BRAIN: 3, STARWARS: 4, FROGS: 3, C5: 5, C9: 9}
PLANES = {BRAIN: 1, STARWARS: 2, FROGS: 1, C5: 2, C9: 3}
# one rule per number of decay planes M, and the deepest pass of its kernels (native.max_generations_depth)
GPU_RULES = {1: BRAIN, 2: STARWARS, 3: C9}
KMAX = {1: 8, 2: 5, 3: 2}
CPU_RULES = [BRAIN, STARWARS, C5, C9]  # C = 3, 4, 5, 9: M = 1, 2, 2, 3
BOUNDARIES = ["torus", "dead"]
BOARDS = [(63, 63), (64, 64), (65, 65), (137, 137), (3, 100)]  # tails of 63, 1 and 9 cells; rows that wrap several times per pass
CPU_DEPTHS = [1, 3, 8]


def board_id(hw):
    return f"{hw[0]}x{hw[1]}"


# Seeds for which the oracle alone satisfies ``lively`` at every depth 1 .. 8 (found with numpy: under Brian's Brain and
# under nine states the 300 cells of the 3 x 100 board lose a state within 17 generations from seed 3100); the other
# boards use 1000 H + W, which does.
SEEDS = {(3, 100, "B2/S/C3", "torus"): 1, (3, 100, "B2/S/C3", "dead"): 1, (3, 100, "B2/S345/C9", "torus"): 1,
         (3, 100, "B2/S345/C9", "dead"): 1}


def seed_of(H, W, rule=None, boundary=None):
    return SEEDS.get((H, W, rule, boundary), 1000 * H + W)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def start_states(H, W, seed, C):
    """A board of random states: half the cells dead, three in ten alive, the rest spread evenly over the dying states."""
    p = [0.5, 0.3] + [0.2 / (C - 2)] * (C - 2)
    return _frozen(np.random.default_rng(seed).choice(C, size=(H, W), p=p).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def history(H, W, seed, rule, boundary, gens):
    """The oracle's boards of generations 0 .. gens, one generation of numpy_generations at a time."""
    b = start_states(H, W, seed, STATES[rule])
    out = [b]
    for _ in range(gens):
        b = _frozen(numpy_generations(b, rule, 1, boundary=boundary))
        out.append(b)
    return out


def lively(H, W, seed, rule, boundary, gens, K, total=None):
    """The oracle alone (module docstring).  ``total``: the generations of the cached history ``gens`` is taken from."""
    h = history(H, W, seed, rule, boundary, total or gens)
    C = STATES[rule]
    ok = set(np.unique(h[gens]).tolist()) == set(range(C))
    if K >= 2:
        ok = ok and any(bool((h[g] >= 2).any()) for g in range(1, gens) if g % K)
    return ok


def check(sim, ref, kernel=None):
    """The simulation's board, state counts and population are the oracle's; ``kernel``: what stats()["kernel"] is."""
    C = sim.states
    got = sim.board()
    assert got.dtype == np.uint8 and got.shape == ref.shape
    bad = got != ref
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} cells differ; first at {tuple(int(v[0]) for v in np.nonzero(bad))}: "
                           f"state {int(got[bad][0])} against {int(ref[bad][0])}")
    counts = sim.state_counts()
    assert counts.dtype == np.uint64 and counts.shape == (C,)
    assert counts.tolist() == np.bincount(ref.ravel(), minlength=C).tolist()
    assert sim.population() == int((ref == 1).sum())
    st = sim.stats()
    assert st["states"] == C and st["rule"] == sim.config.rule
    if kernel is not None:
        assert st["kernel"] == kernel, st["kernel"]


def start_sim(sim, H, W, seed, rule):
    """The simulation at generation 0 on ``start_states``."""
    sim.init(0)
    sim.set_board(start_states(H, W, seed, STATES[rule]))
    return sim


def run_case(make_sim, rule, H, W, boundary, R, K=None, gens=None, kernel=None, **kw):
    """``gens`` generations (default 2R + 1: a full superstep, a second, a remainder) from the random state board on a
    simulation of halo depth R (and pass depth K), checked against the oracle after the first superstep and at the end."""
    seed = seed_of(H, W, rule, boundary)
    gens = 2 * R + 1 if gens is None else gens
    h = history(H, W, seed, rule, boundary, gens)
    assert lively(H, W, seed, rule, boundary, gens, K or R), (rule, H, W, boundary, gens)
    if K is not None:
        kw["kernel_depth"] = K
    s = start_sim(make_sim(H, width=W, rule=rule, boundary=boundary, halo_depth=R, **kw), H, W, seed, rule)
    check(s, h[0], kernel)
    s.step(min(R, gens))
    check(s, h[min(R, gens)], kernel)
    s.step(gens - min(R, gens))
    assert s.generation == gens
    check(s, h[gens], kernel)
    return s
