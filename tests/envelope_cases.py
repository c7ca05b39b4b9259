"""Shared by test_envelope.py (CPU backend) and test_gpu_envelope.py (MI355X): the cases of envelope mode, their numpy
references (``numpy_envelope``, one generation at a time, computed once per board, rule and boundary, kept packed and
read-only) and the checks.

Every check compares ``envelope()`` for exact equality with ``numpy_envelope`` and the final board with the oracle's.
Before a backend is compared, the oracle alone is asked (``lively``): on boards of 63 cells a side or more and passes of
K >= 2 generations the envelope differs from the OR of the boards at the pass ends (generations 0, K, 2K, ... and the
last: a kernel that ORs only its last level could not pass), it differs from the final board and is not all ones, and on
a bounded board the torus oracle gives another envelope."""
import functools

import numpy as np

from gol_amd.ops import numpy_envelope, random_board

CONWAY, HIGHLIFE, REPLICATOR, B1 = "B3/S23", "B36/S23", "B1357/S1357", "B1/S012345678"
RULES = [HIGHLIFE, CONWAY]
BOUNDARIES = ["torus", "dead"]
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8]
SIZES = [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000]
SWEEP_GENS = 2 * max(DEPTHS) + 1


def sweep_rules(boundary):
    """HighLife and Life; on bounded boards also the replicator (dense, but not all ones: asserted by ``lively``)."""
    return RULES + ([REPLICATOR] if boundary == "dead" else [])


class History:
    """Boards and envelopes of generations 0 .. gens, bit-packed; ``board(g)`` / ``envelope(g)`` unpack a fresh array."""

    def __init__(self, start, rule, bounded, gens):
        self.shape = start.shape
        b = np.asarray(start, np.uint8)
        e = numpy_envelope(b, rule, 0, bounded=bounded)
        self._b, self._e = [np.packbits(b)], [np.packbits(e)]
        for _ in range(gens):
            # numpy_envelope over one generation: b | step(b); chained, it is numpy_envelope over all of them
            e1, b = numpy_envelope(b, rule, 1, bounded=bounded, return_board=True)
            e = e | e1
            self._b.append(np.packbits(b))
            self._e.append(np.packbits(e))

    def _un(self, p):
        n = self.shape[0] * self.shape[1]
        return np.unpackbits(p)[:n].reshape(self.shape)

    def board(self, g):
        return self._un(self._b[g])

    def envelope(self, g, start=0):
        """The envelope over generations start .. g."""
        if start == 0:
            return self._un(self._e[g])
        e = self.board(start)
        for k in range(start + 1, g + 1):
            e |= self.board(k)
        return e

    def pass_end_or(self, K, gens):
        """The OR of the boards at generations 0, K, 2K, ... and gens: what ORing only pass results would give."""
        e = self.board(gens)
        for g in range(0, gens, K):
            e |= self.board(g)
        return e


# The replicator and its von Neumann kin keep a 50 % soup at 50 % (they are linear), so over a dozen generations every cell
# has been alive and the envelope is all ones.  Their cases start from a sparse soup, the AND of eight pattern-5 boards
# (one cell in 256), put on the board with set_board(); the other rules start from init(5, seed).
SPARSE_RULES = (REPLICATOR, "B13/S13V")
SWEEP_SEEDS = {64: 65}  # (64 x 64, seed 64: the sparse soup does not reach an edge within 3 generations; chosen with numpy)


def sweep_seed(N):
    return SWEEP_SEEDS.get(N, N)


@functools.lru_cache(maxsize=None)
def start_board(H, W, seed, rule):
    b = random_board(H, W, seed)
    if rule in SPARSE_RULES:
        for i in range(1, 8):
            b = b & random_board(H, W, seed + 1000 * i)
    b.setflags(write=False)
    return b


def start_sim(sim, H, W, seed, rule):
    """The simulation at generation 0 on ``start_board``, its envelope reset to that board."""
    if rule in SPARSE_RULES:
        sim.init(0)
        sim.set_board(start_board(H, W, seed, rule))
    else:
        sim.init(5, seed=seed)
    return sim


@functools.lru_cache(maxsize=None)
def history(H, W, seed, rule, boundary, gens):
    return History(start_board(H, W, seed, rule), rule, boundary == "dead", gens)


def lively(H, W, seed, rule, boundary, gens, K, total=None):
    """The oracle alone (module docstring).  ``total``: the generations of the cached history ``gens`` is taken from."""
    h = history(H, W, seed, rule, boundary, total or gens)
    env = h.envelope(gens)
    ok = not np.array_equal(env, h.board(gens)) and not env.all()
    if K >= 2:
        ok = ok and not np.array_equal(env, h.pass_end_or(K, gens))
    if boundary == "dead":
        ok = ok and not np.array_equal(env, history(H, W, seed, rule, "torus", total or gens).envelope(gens))
    return ok


def report(got, ref):
    bad = np.argwhere(got != ref)
    missing = int(((got == 0) & (ref == 1)).sum())
    return (f"{len(bad)} cells of {got.size} differ ({missing} missing, {len(bad) - missing} extra); first (row, column): "
            f"{bad[0].tolist()}; rows hit: {sorted(set(bad[:, 0].tolist()))[:12]}")


def check(sim, start, env, board, kernel=None):
    """``envelope()`` is ``(start, env)`` exactly, ``stats()`` names the start (and the kernel), the board is ``board``,
    ``envelope_population()`` the oracle's sum.  (One rank: its tile is the board.)"""
    st = sim.stats()
    assert st["envelope"] == start, st
    if kernel is not None:
        assert st["kernel"].startswith(kernel), st
    got_start, got = sim.envelope()
    assert got_start == start and got.dtype == np.uint8 and got.shape == env.shape, (got_start, got.dtype, got.shape, env.shape)
    assert np.array_equal(got, env), report(got, env)
    assert np.array_equal(sim.board(), board)
    assert sim.envelope_population() == int(env.sum())


def run_sweep_case(make_sim, K, N, kernel=None):
    """One depth on one size, the sweep's rules x both boundaries: 2K + 1 generations, a full pass, a second, a remainder
    of 1."""
    gens = 2 * K + 1
    for boundary in BOUNDARIES:
        for rule in sweep_rules(boundary):
            seed = sweep_seed(N)
            h = history(N, N, seed, rule, boundary, SWEEP_GENS)
            if N >= 63:
                assert lively(N, N, seed, rule, boundary, gens, K, SWEEP_GENS), (rule, boundary)
            s = start_sim(make_sim(N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, envelope=True), N, N, seed, rule)
            s.step(gens)
            check(s, 0, h.envelope(gens), h.board(gens), kernel)


def run_multipass_case(make_sim, R, kernel=None, **kw):
    """137 x 200, passes of 8 in supersteps of R, 40 generations; returns the simulations."""
    H, W, gens, seed = 137, 200, 40, 6
    sims = []
    for boundary in BOUNDARIES:
        for rule in RULES:
            h = history(H, W, seed, rule, boundary, gens)
            assert lively(H, W, seed, rule, boundary, gens, 8)
            s = make_sim(H, width=W, rule=rule, boundary=boundary, halo_depth=R, kernel_depth=8, envelope=True, **kw).init(5, seed=seed)
            s.step(gens)
            check(s, 0, h.envelope(gens), h.board(gens), kernel)
            sims.append(s)
    return sims


NBHD_RULES = ["B13/S13V", "B2/S34H"]


def run_nbhd_case(make_sim, rule, K, N, kernel=None):
    gens, seed = 2 * K + 1, 12
    for boundary in BOUNDARIES:
        h = history(N, N, seed, rule, boundary, SWEEP_GENS)
        assert lively(N, N, seed, rule, boundary, gens, K, SWEEP_GENS), (rule, boundary)
        s = start_sim(make_sim(N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, envelope=True), N, N, seed, rule)
        s.step(gens)
        check(s, 0, h.envelope(gens), h.board(gens), kernel)


def run_life_cycle(make_sim, tmp_path, boundary, kernel=None):
    """step(9); step(14); stamps in or and clear mode; envelope_clear(); set_board(); checkpoint / restore; init()."""
    N, rule, seed = 137, HIGHLIFE, 8
    bounded = boundary == "dead"
    h = history(N, N, seed, rule, boundary, 23)
    s = make_sim(N, rule=rule, boundary=boundary, halo_depth=8, envelope=True).init(5, seed=seed)
    check(s, 0, h.board(0), h.board(0), kernel)  # (the init-time timing launches left nothing)
    s.step(9)
    check(s, 0, h.envelope(9), h.board(9))
    s.step(14)
    assert lively(N, N, seed, rule, boundary, 23, 8)
    check(s, 0, h.envelope(23), h.board(23))
    # a stamp in or mode: E |= board, then the run goes on from the stamped board
    env = h.envelope(23)
    s.stamp(np.ones((5, 7), np.uint8), at=(60, 90), mode="or")
    b = s.board()
    assert b[60:65, 90:97].all()
    env = env | b
    check(s, 0, env, b)
    s.step(5)
    e2, b2 = numpy_envelope(b, rule, 5, bounded=bounded, return_board=True)
    env = env | e2
    check(s, 0, env, b2)
    # a stamp in clear mode: the cleared cells stay in E
    block = np.ones((40, 40), np.uint8)
    assert b2[20:60, 30:70].any()
    s.stamp(block, at=(20, 30), mode="clear")
    b3 = s.board()
    assert not b3[20:60, 30:70].any() and env[20:60, 30:70].any()
    check(s, 0, env, b3)
    s.step(3)
    e4, b4 = numpy_envelope(b3, rule, 3, bounded=bounded, return_board=True)
    env = env | e4
    assert env[20:60, 30:70].sum() > e4[20:60, 30:70].sum()  # (cells the stamp removed, still in E)
    check(s, 0, env, b4)
    # envelope_clear(): the new start, E the board
    s.envelope_clear()
    check(s, 31, b4, b4)
    s.step(4)
    e5, b5 = numpy_envelope(b4, rule, 4, bounded=bounded, return_board=True)
    check(s, 31, e5, b5)
    # set_board()
    s.set_board(h.board(2))
    check(s, 35, h.board(2), h.board(2))
    s.step(7)
    check(s, 35, h.envelope(9, start=2), h.board(9))
    # checkpoint / restore: the envelope is not in the file
    s.checkpoint(str(tmp_path / "ck"))
    s.step(2)
    assert s.restore(str(tmp_path / "ck")) == 42
    check(s, s.generation, h.board(9), h.board(9))
    s.step(14)
    check(s, 44, h.envelope(23, start=9), h.board(23))
    # init()
    s.init(5, seed=seed)
    check(s, 0, h.board(0), h.board(0))
    s.step(9)
    check(s, 0, h.envelope(9), h.board(9), kernel)


# Views, on 137 x 200 (tail word: 8 cells)
VIEW_H, VIEW_W, VIEW_SEED, VIEW_GENS = 137, 200, 9, 19


def run_views(make_sim, boundary, windows, wrapping, K=8):
    H, W, gens, rule = VIEW_H, VIEW_W, VIEW_GENS, HIGHLIFE
    h = history(H, W, VIEW_SEED, rule, boundary, gens)
    assert lively(H, W, VIEW_SEED, rule, boundary, gens, K)
    env = h.envelope(gens)
    s = make_sim(H, width=W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, envelope=True).init(5, seed=VIEW_SEED)
    s.step(gens)
    check(s, 0, env, h.board(gens))
    for name, (r0, c0, rows, cols) in windows.items():
        if boundary == "dead" and name in wrapping:
            with_error = None
            try:
                s.envelope_window(r0, c0, rows, cols)
            except ValueError as e:
                with_error = e
            assert with_error is not None and "inside the bounded" in str(with_error), name
            continue
        ref = env[np.ix_((r0 + np.arange(rows)) % H, (c0 + np.arange(cols)) % W)]
        got = s.envelope_window(r0, c0, rows, cols)
        assert got.dtype == np.uint8 and np.array_equal(got, ref), name
        assert np.array_equal(s.window(r0, c0, rows, cols), h.board(gens)[np.ix_((r0 + np.arange(rows)) % H, (c0 + np.arange(cols)) % W)])
    for br, bc in [(8, 64), (137, 256)]:
        ri, ci = np.arange(0, H, br), np.arange(0, W, bc)
        ref = np.add.reduceat(np.add.reduceat(env.astype(np.uint32), ri, axis=0), ci, axis=1)
        got = s.envelope_density(br, bc)
        assert got.dtype == np.uint32 and np.array_equal(got, ref), (br, bc)
    assert np.array_equal(s.envelope_density(64), s.envelope_density(64, 64))
    assert s.envelope_population() == int(env.sum()) and s.population() == int(h.board(gens).sum())


# Rank grids: film_cases.RANK_CASES; 23 generations in two step() calls
RANK_SEED, RANK_GENS = 17, 23  # (the seed wide_cases.run_ranks starts its boards from)


def rank_script(rect):
    def script(s):
        s.step(9).step(RANK_GENS - 9)
        start, cells = s.envelope()
        return start, cells, s.envelope_window(*rect), s.envelope_population(), s.stats()

    return script


def assemble_envelope(H, W, parts):
    full = np.full((H, W), 255, np.uint8)  # (a cell no rank owns stays 255 and fails every comparison)
    for p in parts:
        cells = p.result[1]
        full[p.row0 : p.row0 + cells.shape[0], p.col0 : p.col0 + cells.shape[1]] = cells
    return full


def check_rank_parts(H, W, parts, h, rect):
    env, board = h.envelope(RANK_GENS), h.board(RANK_GENS)
    got = assemble_envelope(H, W, parts)
    assert np.array_equal(got, env), report(got, env)
    full = np.full((H, W), 255, np.uint8)
    for p in parts:
        full[p.row0 : p.row0 + p.board.shape[0], p.col0 : p.col0 + p.board.shape[1]] = p.board
    assert np.array_equal(full, board)
    r0, c0, rows, cols = rect
    ref = env[np.ix_((r0 + np.arange(rows)) % H, (c0 + np.arange(cols)) % W)]
    for p in parts:  # every rank gets the whole window and the global count
        start, _, win, pop, st = p.result
        assert start == 0 and st["envelope"] == 0 and np.array_equal(win, ref) and pop == int(env.sum()), p.rank
