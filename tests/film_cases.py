"""Shared by test_film.py (CPU backend) and test_gpu_film.py (MI355X): the cases of film mode, their numpy references
(``numpy_film``, computed once per board, rule, boundary and window, left read-only) and the checks.

Every check compares ``film()`` for exact equality with ``numpy_film`` and the final board with the oracle's; on boards
of 63 cells a side or more it also asserts that the oracle's frames hold two distinct ones, and on bounded boards that
the torus oracle gives other frames (running the torus could not pass)."""
import functools

import numpy as np

from gol_amd.ops import numpy_film, random_board

HIGHLIFE, B1, REPLICATOR = "B36/S23", "B1/S012345678", "B1357/S1357"
RULES = [HIGHLIFE, B1]  # B1 puts births just outside every edge of a bounded board at every level of a pass
BOUNDARIES = ["torus", "dead"]
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8]
SIZES = [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000]
SWEEP_GENS = 2 * max(DEPTHS) + 1


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frames_of(H, W, seed, rule, boundary, gens, rect):
    """``numpy_film`` of the H x W pattern-5 board of ``seed``: the frames of generations 1 .. gens."""
    return _frozen(numpy_film(random_board(H, W, seed), rule, gens, rect, bounded=boundary == "dead"))


def boards_of(H, W, seed, rule, boundary, gens):
    """The boards after generations 1 .. gens: the film of the whole board."""
    return frames_of(H, W, seed, rule, boundary, gens, (0, 0, H, W))


def sweep_rect(N, boundary):
    """The whole board: on the torus from (N // 3, N // 2 + 1), across both seams; on a bounded board at (0, 0)."""
    return (N // 3, N // 2 + 1, N, N) if boundary == "torus" else (0, 0, N, N)


def distinct(H, W, seed, rule, boundary, gens, rect, first=0):
    """The oracle alone: its frames hold two distinct ones."""
    return len({f.tobytes() for f in frames_of(H, W, seed, rule, boundary, gens, rect)[first:]}) >= 2


def told_apart(H, W, seed, rule, gens, rect, first=0):
    """The oracle alone: the bounded board's frames are not the torus's (the window is within reach of an edge)."""
    return not np.array_equal(frames_of(H, W, seed, rule, "dead", gens, rect)[first:],
                              frames_of(H, W, seed, rule, "torus", gens, rect)[first:])


def lively(H, W, seed, rule, boundary, gens, rect, first=0):
    """Two distinct frames, and on a bounded board frames the torus does not give."""
    return distinct(H, W, seed, rule, boundary, gens, rect, first) and (
        boundary == "torus" or told_apart(H, W, seed, rule, gens, rect, first))


def check(sim, start, ref, board, rect, kernel=None):
    """``film()`` is ``(start, ref)`` exactly, ``stats()`` names the window (and the kernel), the board is ``board``."""
    st = sim.stats()
    assert st["film"] == tuple(rect), st
    if kernel is not None:
        assert st["kernel"].startswith(kernel), st
    got_start, got = sim.film()
    assert got_start == start and got.dtype == np.uint8 and got.shape == ref.shape, (got_start, got.dtype, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"{len(bad)} cells of {got.size} differ; first (frame, row, column): {bad[0].tolist()}; "
                             f"frames hit: {sorted(set(bad[:, 0].tolist()))[:12]}")
    assert np.array_equal(sim.board(), board)


def run_sweep_case(make_sim, K, N, kernel=None):
    """One depth on one size, two rules x both boundaries: 2K + 1 generations, a full superstep and the remainders."""
    gens = 2 * K + 1
    for boundary in BOUNDARIES:
        rect = sweep_rect(N, boundary)
        for rule in RULES:
            ref = frames_of(N, N, N, rule, boundary, SWEEP_GENS, rect)[:gens]
            board = boards_of(N, N, N, rule, boundary, SWEEP_GENS)[gens - 1]
            if N >= 63:
                assert lively(N, N, N, rule, boundary, SWEEP_GENS, rect)
                assert len({f.tobytes() for f in ref}) >= 2
            s = make_sim(N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, film=rect).init(5, seed=N)
            s.step(gens)
            check(s, 0, ref, board, rect, kernel)


# Window shapes on 137 x 200 (tail word: 8 cells): (r0, c0, rows, cols); those that wrap run on the torus only
SHAPE_H, SHAPE_W, SHAPE_SEED, SHAPE_GENS = 137, 200, 9, 19
WINDOWS = {
    "cell": (70, 131, 1, 1),
    "in_word": (30, 70, 9, 5),
    "cols_60_69": (100, 60, 20, 10),
    "full_row": (136, 0, 1, 200),
    "full_column": (0, 199, 137, 1),
    "rows_wrap": (130, 20, 15, 40),
    "cols_wrap_tail": (5, 190, 30, 21),
}
WRAPPING = ("rows_wrap", "cols_wrap_tail")
AT_EDGE = ("full_row", "full_column")  # within reach of a bounded board's edge: the torus gives other frames
WINDOW_RULES = [HIGHLIFE, REPLICATOR]  # (B1/S012345678 fills a small window within a few generations)


def run_window_case(make_sim, name, K, kernel=None):
    rect = WINDOWS[name]
    H, W = SHAPE_H, SHAPE_W
    for boundary in BOUNDARIES:
        if boundary == "dead" and name in WRAPPING:
            continue
        for rule in WINDOW_RULES:
            ref = frames_of(H, W, SHAPE_SEED, rule, boundary, SHAPE_GENS, rect)
            board = boards_of(H, W, SHAPE_SEED, rule, boundary, SHAPE_GENS)[-1]
            assert distinct(H, W, SHAPE_SEED, rule, boundary, SHAPE_GENS, rect)
            if boundary == "dead" and name in AT_EDGE:
                assert told_apart(H, W, SHAPE_SEED, rule, SHAPE_GENS, rect)
            s = make_sim(H, width=W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, film=rect).init(5, seed=SHAPE_SEED)
            s.step(SHAPE_GENS)
            check(s, 0, ref, board, rect, kernel)


# Rank grids: (P, grid keywords, H, W, windows); the first window of each lies over the point where tiles meet
RANK_SEED, RANK_GENS = 17, 23  # (the seed wide_cases.run_ranks starts its boards from)
RANK_CASES = {
    "1d3": (3, {}, 96, 128, [(28, 50, 10, 30), (90, 120, 12, 16)]),
    # (strips of 100 rows: an interior beside two 16-row bands, so the split schedule can run; the second window
    # crosses a rank boundary, the y seam and, through the 8-cell tail word, the x seam)
    "1d4": (4, {}, 400, 200, [(190, 60, 30, 70), (395, 180, 110, 40)]),
    "2x2": (4, {"decomp": "2d", "grid": "2x2"}, 128, 256, [(60, 120, 9, 17), (100, 250, 50, 20)]),
    # (nine ranks; inside the centre rank)
    "3x3": (9, {"decomp": "2d", "grid": "3x3"}, 96, 192, [(20, 50, 60, 100), (40, 70, 8, 40)]),
}


def inside(rect, H, W):
    return rect[0] >= 0 and rect[1] >= 0 and rect[0] + rect[2] <= H and rect[1] + rect[3] <= W


def rank_windows(name, boundary):
    _, _, H, W, windows = RANK_CASES[name]
    return [r for r in windows if boundary == "torus" or inside(r, H, W)]


def rank_ref(name, rule, boundary, rect):
    _, _, H, W, _ = RANK_CASES[name]
    return (frames_of(H, W, RANK_SEED, rule, boundary, RANK_GENS, rect),
            boards_of(H, W, RANK_SEED, rule, boundary, RANK_GENS)[-1])


def film_script(s):
    """Several step() calls; every rank returns its film and its stats."""
    s.step(9).step(RANK_GENS - 9)
    start, frames = s.film()
    return start, frames, s.stats()
