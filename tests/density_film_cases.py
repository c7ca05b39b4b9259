"""Shared by test_density_film.py (CPU backend) and test_gpu_density_film.py (MI355X): the cases of density-film mode,
their numpy references (``numpy_density_film``, computed once per board, rule, boundary and block shape, left
read-only) and the checks.

Every check compares ``density_film()`` for exact equality with ``numpy_density_film``, the sum of every map with the
population of the oracle's board of that generation, and the final board with the oracle's; before the engine runs, on
boards of 63 cells a side or more it asserts that the oracle's HighLife maps hold two distinct ones, and on bounded
boards that the torus oracle gives other maps (running the torus could not pass).  The boards are pattern-5 boards:
ghost rows and ghost words stay live, so a cell counted twice or missed changes a number."""
import functools
import os
import subprocess

import numpy as np

import film_cases as fc
from gol_amd.ops import numpy_density_film, random_board

HIGHLIFE, B1, REPLICATOR = fc.HIGHLIFE, fc.B1, fc.REPLICATOR
RULES = [HIGHLIFE, B1]  # B1 puts births just outside every edge of a bounded board at every level of a pass
BOUNDARIES = fc.BOUNDARIES
DEPTHS = fc.DEPTHS
SIZES = fc.SIZES
SWEEP_GENS = fc.SWEEP_GENS
WHOLE = "whole"  # one block: (H, ceil(W / 64) * 64); the map is the census
# (1, 64): a counter per word, flushed every row.  (7, 64): block ends out of step with K, segments and tiles.
SWEEP_BLOCKS = [(1, 64), (7, 64), (8, 128), (64, 64), (50, 192), WHOLE]


def blocks_of(blocks, H, W):
    return (H, -(-W // 64) * 64) if blocks == WHOLE else tuple(blocks)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def maps_of(H, W, seed, rule, boundary, gens, blocks):
    """``numpy_density_film`` of the H x W pattern-5 board of ``seed``: the maps of generations 1 .. gens."""
    return _frozen(numpy_density_film(random_board(H, W, seed), rule, gens, blocks, bounded=boundary == "dead"))


boards_of = fc.boards_of  # the oracle's boards after generations 1 .. gens (shared with the film tests)


def distinct(H, W, seed, rule, boundary, gens, blocks, first=0, upto=None):
    """The oracle alone: its maps of generations first + 1 .. upto (default: all ``gens``) hold two distinct ones."""
    return len({m.tobytes() for m in maps_of(H, W, seed, rule, boundary, gens, blocks)[first:upto]}) >= 2


def told_apart(H, W, seed, rule, gens, blocks, first=0, upto=None):
    """The oracle alone: the bounded board's maps of those generations are not the torus's."""
    return not np.array_equal(maps_of(H, W, seed, rule, "dead", gens, blocks)[first:upto],
                              maps_of(H, W, seed, rule, "torus", gens, blocks)[first:upto])


def lively(H, W, seed, rule, boundary, gens, blocks, upto=None):
    """What the tests assert of the oracle before the engine runs, on boards of 63 cells a side or more, of the maps
    the engine is compared with (the first ``upto`` of the ``gens`` the oracle computed; default: all): on a bounded
    board the torus gives other maps; under HighLife two maps differ.  (B1/S012345678 fills a small torus in one
    generation, and its maps are constant from then on: no distinct maps are asked of it.  On a 1 x 1 board that rule
    keeps a live cell and leaves a dead one dead on either boundary, so nothing is asked of the 1-, 2- and 3-cell
    boards.)"""
    if min(H, W) < 63:
        return True
    if boundary == "dead" and not told_apart(H, W, seed, rule, gens, blocks, upto=upto):
        return False
    return rule != HIGHLIFE or distinct(H, W, seed, rule, boundary, gens, blocks, upto=upto)


def check(sim, start, ref, boards, blocks, kernel=None):
    """``density_film()`` is ``(start, ref)`` exactly, every map sums to the population of its board (``boards[i]`` the
    oracle's board of map i), ``stats()`` names the blocks (and the kernel), the board is ``boards[-1]``."""
    st = sim.stats()
    assert st["density_film"] == tuple(blocks), st
    if kernel is not None:
        assert st["kernel"].startswith(kernel), st
    got_start, got = sim.density_film()
    assert got_start == start and got.dtype == np.uint32 and got.shape == ref.shape, (got_start, got.dtype, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        g, i, j = bad[0].tolist()
        raise AssertionError(f"{len(bad)} counts of {got.size} differ; first (map, block row, block column): {[g, i, j]}: "
                             f"{int(got[g, i, j])} against {int(ref[g, i, j])}; maps hit: {sorted(set(bad[:, 0].tolist()))[:12]}; "
                             f"sums of map {g}: {int(got[g].sum())} against {int(ref[g].sum())}")
    assert len(boards) == len(ref)
    pops = np.asarray(boards).reshape(len(boards), -1).sum(axis=1, dtype=np.uint64)
    assert np.array_equal(got.reshape(len(got), -1).sum(axis=1, dtype=np.uint64), pops)
    assert np.array_equal(sim.board(), boards[-1])


def sweep_blocks(K, N):
    """The block shapes of the four sub-cases (boundary x rule) of a sweep case: they cycle with the case; at 137 and
    1000 every depth meets (7, 64) and (64, 64) on both boundaries."""
    if N in (137, 1000):
        return [(7, 64), (64, 64), (64, 64), (7, 64)]
    at = K + SIZES.index(N)
    return [SWEEP_BLOCKS[(at + j) % len(SWEEP_BLOCKS)] for j in range(4)]


def run_sweep_case(make_sim, K, N, kernel=None):
    """One depth on one size, two rules x both boundaries: 2K + 1 generations, a full superstep and the remainders."""
    gens = 2 * K + 1
    shapes = iter(sweep_blocks(K, N))
    for boundary in BOUNDARIES:
        for rule in RULES:
            blocks = blocks_of(next(shapes), N, N)
            assert lively(N, N, N, rule, boundary, SWEEP_GENS, blocks, upto=gens)
            ref = maps_of(N, N, N, rule, boundary, SWEEP_GENS, blocks)[:gens]
            boards = boards_of(N, N, N, rule, boundary, SWEEP_GENS)[:gens]
            s = make_sim(N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, density_film=blocks).init(5, seed=N)
            s.step(gens)
            check(s, 0, ref, boards, blocks, kernel)


# Block shapes on 137 x 200 (tail word: 8 cells); (200, 64): a block taller than the board
SHAPE_H, SHAPE_W, SHAPE_SEED, SHAPE_GENS = 137, 200, 9, 19
SHAPE_BLOCKS = [(1, 64), (5, 64), (137, 256), (200, 64)]
SHAPE_RULES = [HIGHLIFE, REPLICATOR]


def run_shape_case(make_sim, blocks, K, kernel=None, rules=SHAPE_RULES, seed=SHAPE_SEED, gens=SHAPE_GENS):
    H, W = SHAPE_H, SHAPE_W
    for boundary in BOUNDARIES:
        for rule in rules:
            assert distinct(H, W, seed, rule, boundary, gens, blocks)
            assert boundary == "torus" or told_apart(H, W, seed, rule, gens, blocks)
            ref = maps_of(H, W, seed, rule, boundary, gens, blocks)
            boards = boards_of(H, W, seed, rule, boundary, gens)
            s = make_sim(H, width=W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, density_film=blocks).init(5, seed=seed)
            s.step(gens)
            check(s, 0, ref, boards, blocks, kernel)


# Rank grids: the shapes of film_cases.RANK_CASES.  The ranks' rows meet at multiples of 32 (1d3, 3x3), 100 (1d4) and
# at 64 (2x2): none is a multiple of 7 or 27, so with (7, 64) and (27, 192) no boundary between rows of ranks is a
# block-row boundary and ranks add into the same blocks; with (20, 128) that holds in 1d3, 2x2 and 3x3, while the
# strips of 1d4 end where block rows end.  Columns of ranks meet at multiples of 64: boundaries of 64-column blocks,
# and at 128 (2x2) of 128-column blocks; with 192-column blocks the two columns of the 2x2 grid share the first block
# column and the three of the 3x3 grid (64, 128) the only one.
RANK_CASES = fc.RANK_CASES
RANK_SEED, RANK_GENS = fc.RANK_SEED, fc.RANK_GENS
RANK_BLOCKS = [(7, 64), (20, 128), (27, 192)]


def rank_ref(name, rule, boundary, blocks):
    _, _, H, W, _ = RANK_CASES[name]
    return (maps_of(H, W, RANK_SEED, rule, boundary, RANK_GENS, blocks), boards_of(H, W, RANK_SEED, rule, boundary, RANK_GENS))


def film_script(s):
    """Several step() calls; every rank returns its maps and its stats."""
    s.step(9).step(RANK_GENS - 9)
    start, maps = s.density_film()
    return start, maps, s.stats()


def check_rank_parts(parts, ref, boards, blocks):
    """Every rank returns the same whole array, the oracle's; every map sums to its board's population."""
    pops = np.asarray(boards).reshape(len(boards), -1).sum(axis=1, dtype=np.uint64)
    for p in parts:
        start, maps, st = p.result
        assert start == 0 and st["density_film"] == tuple(blocks), (p.rank, start, st)
        assert maps.dtype == np.uint32 and np.array_equal(maps, ref), p.rank
        assert np.array_equal(maps.reshape(len(maps), -1).sum(axis=1, dtype=np.uint64), pops), p.rank


# ----- the CLI -----

CLI_CLEARED = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_BOUNDARY",
               "GOL_PATTERN_FILE", "GOL_PATTERN_AT", "GOL_RLE_OUT", "GOL_CENSUS", "GOL_CENSUS_OUT", "GOL_COMPAT", "GOL_SUBTILES",
               "GOL_SIGNATURE", "GOL_SIGNATURE_OUT", "GOL_FILM", "GOL_FILM_OUT", "GOL_DENSITY_FILM", "GOL_DENSITY_FILM_OUT",
               "GOL_DENSITY_FILM_MB", "GOL_KERNEL")


def cli(gol_bin, args, cwd, backend="cpu", **env):
    e = dict(os.environ)
    for k in CLI_CLEARED:
        e.pop(k, None)
    e["GOL_BACKEND"] = backend
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=300)
