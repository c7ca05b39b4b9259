"""Shared by test_signature.py (CPU) and test_gpu_signature.py (MI355X): the boards find_cycle() is tried on, and their
oracle, a brute-force numpy loop over a dict of ``board.tobytes()``.

The condition on the inputs is that the oracle itself cycles within ``max_generations``.  The chunks are not
multiples of the periods, and the blinker's (3) is below the engines' pass depth."""
import functools

import numpy as np

from gol_amd.ops import Cycle, numpy_step_rule, numpy_step_rule_bounded

GLIDER_CELLS = [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)]


def brute_force_cycle(board, rule, bounded, max_generations):
    """(transient, period, boards of the cycle) by a dict of board bytes; None when nothing repeats in time."""
    step = numpy_step_rule_bounded if bounded else numpy_step_rule
    b = np.asarray(board, np.uint8)
    seen, boards = {b.tobytes(): 0}, [b]
    for g in range(1, max_generations + 1):
        b = step(b, rule, 1)
        prev = seen.get(b.tobytes())
        if prev is not None:
            return prev, g - prev, boards[prev:]
        seen[b.tobytes()] = g
        boards.append(b)
    return None


def place(H, W, cells, at=(0, 0)):
    b = np.zeros((H, W), np.uint8)
    for r, c in cells:
        b[at[0] + r, at[1] + c] = 1
    return b


R_PENTOMINO = [(0, 1), (0, 2), (1, 0), (1, 1), (2, 1)]
# name: (board, rule, boundary, max_generations, chunk)
CYCLE_CASES = {
    "blinker-8": (place(8, 8, [(3, 2), (3, 3), (3, 4)]), "B3/S23", "torus", 4096, 3),
    "glider-64": (place(64, 64, GLIDER_CELLS, (10, 10)), "B3/S23", "torus", 4096, 100),
    "glider-65x130": (place(65, 130, GLIDER_CELLS, (10, 10)), "B3/S23", "torus", 4096, 7),
    "glider-64-dead": (place(64, 64, GLIDER_CELLS, (10, 10)), "B3/S23", "dead", 4096, 50),
    "rpent-64": (place(64, 64, R_PENTOMINO, (30, 30)), "B3/S23", "torus", 4096, 255),
    "rpent-137-dead": (place(137, 137, R_PENTOMINO, (60, 60)), "B3/S23", "dead", 4096, 300),
    "b2s-16": (place(16, 16, [(5, 5), (5, 6)]), "B2/S", "torus", 4096, 37),
    "dies-out": (place(32, 32, [(4, 4), (4, 5)]), "B3/S23", "torus", 64, 5),
    "glider-128": (place(128, 128, GLIDER_CELLS, (10, 10)), "B3/S23", "torus", 4096, 100),  # (wide enough for a 2 x 2 grid)
}
# the cases a 2 x 2 rank grid can hold: two words or more per row, and on the torus a width that is a multiple of 64
GRID_CASES = [n for n, c in CYCLE_CASES.items() if c[0].shape[1] >= 128 and (c[2] == "dead" or c[0].shape[1] % 64 == 0)]


@functools.lru_cache(maxsize=None)
def cycle_oracle(name):
    board, rule, boundary, max_generations, _ = CYCLE_CASES[name]
    return brute_force_cycle(board, rule, boundary == "dead", max_generations)


def check_cycle(sim, name, got):
    """`got` against the brute-force oracle: transient and period equal, the final board the oracle's board of that
    generation, and its population."""
    transient, period, boards = cycle_oracle(name)
    assert isinstance(got, Cycle) and (got.transient, got.period) == (transient, period), (name, got, transient, period)
    assert got.generation == sim.generation >= transient + period
    want = boards[(got.generation - transient) % period]
    assert got.population == int(want.sum()) == sim.population()
    return want
