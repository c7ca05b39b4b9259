"""Shared by test_ltl.py (CPU backend) and test_gpu_ltl.py (MI355X): the cases of the Larger than Life rules, their
numpy references (``numpy_ltl``, computed once per board, rule and boundary, kept read-only) and the checks.

Every comparison is exact.  The start board is a density gradient, so that every count from 0 to (2R+1)^2 occurs:
with ``L = max(H, W)`` a cell (r, c) is alive iff ``default_rng(seed).random((H, W)) < ((r + c) mod L) / (L - 1)``.
(A uniform random soup dies within three generations under these rules on most shapes.)

Before a backend is compared the oracle alone is asked (``preconditions``):
  * the thresholds are exercised on the start board: among dead cells the counts bmin - 1, bmin, bmax and bmax + 1 all
    occur, among live cells smin - 1, smin, smax and smax + 1, each where a cell of that state can have that count, so
    an off-by-one in any comparator cannot pass;
  * each of the two generations changes the board, and the board is neither empty nor full;
  * on a bounded board the result differs from the torus result, after each generation.
"""
import functools

import numpy as np

from gol_amd.ops import numpy_ltl, parse_ltl_rule

# Two rules per range: Bosco's rule scaled to the box (M1), and an M0 twin with the same B.
_M1 = {1: "S3..4,B3..3", 2: "S7..12,B7..9", 3: "S14..23,B14..18", 4: "S23..39,B23..30", 5: "S34..58,B34..45",
       6: "S47..81,B47..63", 7: "S63..108,B63..84"}
_M0_S = {1: "S2..4", 2: "S7..12", 3: "S13..23", 4: "S22..38", 5: "S33..57", 6: "S46..80", 7: "S61..106"}
RANGES = [1, 2, 3, 4, 5, 6, 7]
BOUNDARIES = ["torus", "dead"]
GENS = 2  # compared after each one: both buffer directions


def rule_m1(R):
    return f"R{R},C0,M1,{_M1[R]},NM"


def rule_m0(R):
    return f"R{R},C0,M0,{_M0_S[R]},{_M1[R].split(',')[1]},NM"


def rules(R):
    return [rule_m1(R), rule_m0(R)]


BOSCO = rule_m1(5)
SQUARES = [(63, 63), (64, 64), (65, 65), (137, 137)]  # tail words of 63, 1 and 9 cells, packed segments


def shapes(R):
    """The squares, and a board of 2R + 1 rows on which every window wraps around all rows."""
    return SQUARES + [(2 * R + 1, 1000)]


WIDE_RANGES = [1, 5, 7]  # the wide shapes of wide_cases (64 x 3968, 64 x 3950) run for these


def board_id(hw):
    return f"{hw[0]}x{hw[1]}"


# Seeds other than 1000 H + W: where that seed fails a precondition, the next seed (1, 2, ...) that passes all three
# (found with numpy; run_case asserts the preconditions for every case it runs).  On the torus of 15 x 1000 cells seed
# 15000 + 1000 misses a threshold count under both R = 7 rules; every other case passes with 1000 H + W.
SEEDS = {(15, 1000, rule_m1(7), "torus"): 1, (15, 1000, rule_m0(7), "torus"): 1}


def seed_of(H, W, rule, boundary):
    return SEEDS.get((H, W, rule, boundary), 1000 * H + W)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def start_board(H, W, seed):
    L = max(H, W)
    r, c = np.indices((H, W))
    p = ((r + c) % L) / (L - 1)
    return _frozen((np.random.default_rng(seed).random((H, W)) < p).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def history(H, W, seed, rule, boundary, gens=GENS):
    """The oracle's boards of generations 0 .. gens, one generation of numpy_ltl at a time."""
    b = start_board(H, W, seed)
    out = [b]
    for _ in range(gens):
        b = _frozen(numpy_ltl(b, rule, 1, boundary=boundary))
        out.append(b)
    return out


def counts(board, rule, boundary):
    """Golly's n of every cell: the live cells of the box, the cell itself counted iff M is 1."""
    R, M = parse_ltl_rule(rule)[:2]
    H, W = board.shape
    live = board.astype(np.int32)
    if boundary == "torus":
        n = sum(np.roll(np.roll(live, dy, axis=0), dx, axis=1) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
    else:
        pad = np.zeros((H + 2 * R, W + 2 * R), dtype=np.int32)
        pad[R : R + H, R : R + W] = live
        n = sum(pad[dy : dy + H, dx : dx + W] for dy in range(2 * R + 1) for dx in range(2 * R + 1))
    return n if M else n - live


def thresholds_exercised(H, W, seed, rule, boundary):
    R, M, smin, smax, bmin, bmax = parse_ltl_rule(rule)
    b = start_board(H, W, seed)
    n = counts(b, rule, boundary)
    box = (2 * R + 1) ** 2
    dead_n, live_n = set(np.unique(n[b == 0]).tolist()), set(np.unique(n[b == 1]).tolist())
    # what a cell of each state can count: a dead centre leaves box - 1 cells; a live one is counted iff M
    dead_ok = lambda v: 0 <= v <= box - 1  # noqa: E731
    live_ok = (lambda v: 1 <= v <= box) if M else (lambda v: 0 <= v <= box - 1)
    return all(v in dead_n for v in (bmin - 1, bmin, bmax, bmax + 1) if dead_ok(v)) and all(
        v in live_n for v in (smin - 1, smin, smax, smax + 1) if live_ok(v)
    )


def lively(H, W, seed, rule, boundary, gens=GENS):
    h = history(H, W, seed, rule, boundary, gens)
    return all(not np.array_equal(h[g], h[g + 1]) and 0 < int(h[g + 1].sum()) < h[g + 1].size for g in range(gens))


def bounded_differs(H, W, seed, rule, gens=GENS):
    t, d = history(H, W, seed, rule, "torus", gens), history(H, W, seed, rule, "dead", gens)
    return all(not np.array_equal(t[g], d[g]) for g in range(1, gens + 1))


def preconditions(H, W, seed, rule, boundary, gens=GENS):
    """The oracle alone (module docstring)."""
    return (thresholds_exercised(H, W, seed, rule, boundary) and lively(H, W, seed, rule, boundary, gens)
            and bounded_differs(H, W, seed, rule, gens))


def check(sim, ref, kernel=None):
    """The simulation's board and population are the oracle's; ``kernel``: what stats()["kernel"] is."""
    got = sim.board()
    assert got.dtype == np.uint8 and got.shape == ref.shape
    bad = got != ref
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} cells differ; first at {tuple(int(v[0]) for v in np.nonzero(bad))}; "
                           f"rows {sorted(set(np.nonzero(bad)[0].tolist()))[:8]}, columns {sorted(set(np.nonzero(bad)[1].tolist()))[:8]}")
    assert sim.population() == int(ref.sum())
    st = sim.stats()
    assert st["states"] == 2 and st["rule"] == sim.config.rule and st["depth"] == 1 and st["kernel_depth"] == 1, st
    if kernel is not None:
        assert st["kernel"] == kernel, st["kernel"]


def start_sim(sim, H, W, seed):
    """The simulation at generation 0 on ``start_board``."""
    sim.init(0)
    sim.set_board(start_board(H, W, seed))
    return sim


def run_case(make_sim, rule, H, W, boundary, gens=GENS, kernel=None, **kw):
    """``gens`` generations from the gradient board, checked against the oracle after each one."""
    seed = seed_of(H, W, rule, boundary)
    assert preconditions(H, W, seed, rule, boundary, gens), (rule, H, W, boundary, seed)
    h = history(H, W, seed, rule, boundary, gens)
    s = start_sim(make_sim(H, width=W, rule=rule, boundary=boundary, **kw), H, W, seed)
    check(s, h[0], kernel)
    for g in range(1, gens + 1):
        s.step(1)
        assert s.generation == g
        check(s, h[g], kernel)
    return s
