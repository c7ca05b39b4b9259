"""Shared cases of the soup-batch tests (test_soups.py: CPU backend, oracle, CLI; test_gpu_soups.py: HIP backend).

Every expectation comes from the byte-per-cell oracle ``numpy_soup_settle`` / ``numpy_step_rule``; an oracle result is
computed once per (board, rule) and shared by all tests of both files.  The facts about the random soups (which settle,
by when) were established with the oracle alone; the tests assert them of the oracle before comparing the backend.
"""
import functools

import numpy as np

from gol_amd.ops import numpy_soup_settle, numpy_step_rule, random_board

SEED = 1000
STEP_RULES = ["B3/S23", "B36/S23", "B3678/S34678"]  # (B8 and S8 are leaves of the generic finish)
STEP_GENS = [1, 2, 3, 17]                            # cumulative: generations 1, 3, 6, 23
MAX_GENS = 20000

# (size, rule, number of soups from SEED on): the random soups that settle, a subset the oracle does in seconds
SETTLING = [(64, "B3/S23", 8), (128, "B3/S23", 2), (64, "B36/S23", 4)]
# every soup of these is found by this generation (the save schedule: 2^k + 1)
FOUND_BY = {(64, "B3/S23"): 8193, (128, "B3/S23"): 4097, (64, "B36/S23"): 2049}


@functools.lru_cache(maxsize=None)
def soup(S, seed):
    b = random_board(S, S, seed)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def settled(S, rule, seed, max_gens=MAX_GENS):
    """The oracle's (period, transient, generation, population, board) of the random soup ``seed``."""
    return numpy_soup_settle(soup(S, seed), rule, max_gens, transient=True)


def patterns(S):
    """The seam patterns of a soup of side S, by name."""
    def board(cells):
        b = np.zeros((S, S), dtype=np.uint8)
        for r, c in cells:
            b[r % S, c % S] = 1
        return b

    out = {
        "blinker_rows_seam": board([(S - 1, 10), (0, 10), (1, 10)]),          # vertical, across rows S-1 / 0
        "blinker_cols_seam": board([(20, S - 2), (20, S - 1), (20, 0)]),      # horizontal, across columns S-1 / 0
        "corner_block": board([(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]),
        "empty": board([]),
        "glider": board([(1, 2), (2, 3), (3, 1), (3, 2), (3, 3)]),
    }
    if S == 128:
        out["blinker_word_seam"] = board([(40, 62), (40, 63), (40, 64)])     # across the word seam 63 | 64
    return out


@functools.lru_cache(maxsize=None)
def pattern_oracle(S, name):
    return numpy_soup_settle(patterns(S)[name], "B3/S23", 4 * S * 4, transient=True)


def records_of(oracles):
    """Oracle tuples -> the four arrays of a SoupResult."""
    return (
        np.array([o[0] for o in oracles], dtype=np.uint32),
        np.array([o[1] for o in oracles], dtype=np.int64),
        np.array([o[2] for o in oracles], dtype=np.uint32),
        np.array([o[3] for o in oracles], dtype=np.uint32),
    )


def assert_result(res, boards, oracles):
    exp = records_of(oracles)
    for name, got, want in zip(("period", "transient", "generation", "population"), res, exp):
        assert got.dtype == want.dtype, name
        assert np.array_equal(got, want), (name, got, want)
    assert boards.dtype == np.uint8
    assert np.array_equal(boards, np.stack([o[4] for o in oracles]))


# ---- the cases, run by both files with their backend ----------------------------------------------------------------

def check_plain_steps(gol, backend, S, rule):
    n = 5
    sb = gol.SoupBatch(n, S, rule, backend=backend, seed=SEED)
    ref = [soup(S, SEED + i) for i in range(n)]
    assert np.array_equal(sb.boards(), np.stack(ref))
    total = 0
    for g in STEP_GENS:
        sb.step(g)
        total += g
        ref = [numpy_step_rule(b, rule, g) for b in ref]
        got = sb.boards()
        for i in range(n):
            assert np.array_equal(got[i], ref[i]), (S, rule, total, i, int((got[i] != ref[i]).sum()))
    rec = sb.records()
    assert list(rec.generation) == [total] * n and list(rec.period) == [0] * n and list(rec.transient) == [-1] * n
    assert list(rec.population) == [int(b.sum()) for b in ref]
    assert sb.stats()["kernel"] == f"soups@{S}" + ("" if rule == "B3/S23" else ":rule")


def check_patterns(gol, backend, S):
    pats = patterns(S)
    names = list(pats)
    oracles = [pattern_oracle(S, k) for k in names]
    o = dict(zip(names, oracles))
    assert o["empty"][:3] == (1, 0, 1) and o["corner_block"][:3] == (1, 0, 1)
    assert o["glider"][:3] == (4 * S, 0, 8 * S - 1)  # the save at 4 S - 1 is on the cycle: found at 511 / 1023
    sb = gol.SoupBatch.from_boards(np.stack([pats[k] for k in names]), backend=backend)
    res = sb.settle(16 * S, transient=True)
    assert_result(res, sb.boards(), oracles)
    g = names.index("glider")
    assert (res.period[g], res.transient[g], res.generation[g]) == (4 * S, 0, {64: 511, 128: 1023}[S])
    for k in ("empty", "corner_block"):
        assert (res.period[names.index(k)], res.transient[names.index(k)]) == (1, 0)


def settling_oracles(S, rule, n):
    oracles = [settled(S, rule, SEED + i) for i in range(n)]
    assert all(o[0] > 0 and o[1] >= 0 and o[2] <= FOUND_BY[(S, rule)] for o in oracles)  # every soup settles
    return oracles


def check_settling(gol, backend, S, rule, n):
    oracles = settling_oracles(S, rule, n)
    sb = gol.SoupBatch(n, S, rule, backend=backend, seed=SEED)
    res = sb.settle(MAX_GENS, transient=True)
    assert_result(res, sb.boards(), oracles)
    assert (res.period > 0).all() and sb.stats()["settled"] == n


def check_unsettled(gol, backend):
    n, gens = 3, 300
    sb = gol.SoupBatch(n, 64, "B2/S", backend=backend, seed=SEED)
    res = sb.settle(gens, transient=True)
    assert list(res.period) == [0] * n and list(res.generation) == [gens] * n and list(res.transient) == [-1] * n
    ref = np.stack([numpy_step_rule(soup(64, SEED + i), "B2/S", gens) for i in range(n)])
    assert np.array_equal(sb.boards(), ref)
    assert list(res.population) == [int(b.sum()) for b in ref]
    assert sb.stats()["settled"] == 0


def check_chunks(gol, backend, S, rule, n):
    oracles = settling_oracles(S, rule, n)
    for chunk in (1, 7, 4096):
        sb = gol.SoupBatch(n, S, rule, backend=backend, seed=SEED)
        assert_result(sb.settle(MAX_GENS, transient=True, chunk=chunk), sb.boards(), oracles)
    sb = gol.SoupBatch(n, S, rule, backend=backend, seed=SEED)
    first = sb.settle(100)
    assert (first.generation <= 100).all() and (first.transient == -1).all()
    sb.settle(1000, transient=True)
    assert_result(sb.settle(MAX_GENS, transient=True), sb.boards(), oracles)


def check_mixed(gol, backend, chunk=512):
    """Empty boards, gliders and random soups interleaved: waves of one launch end at generations 1, 511 and later."""
    S, k = 64, 3
    pats = patterns(S)
    boards, oracles = [], []
    for i in range(k):
        boards += [pats["empty"], pats["glider"], soup(S, SEED + i)]
        oracles += [pattern_oracle(S, "empty"), pattern_oracle(S, "glider"), settled(S, "B3/S23", SEED + i)]
    sb = gol.SoupBatch.from_boards(np.stack(boards), backend=backend)
    res = sb.settle(MAX_GENS, transient=True, chunk=chunk)
    assert_result(res, sb.boards(), oracles)
    assert sb.stats()["launches"] > 1 and sb.stats()["settled"] == 3 * k
    return sb


def csv_lines(oracles):
    return ["soup,period,transient,generation,population"] + [
        f"{i},{o[0]},{o[1]},{o[2]},{o[3]}" for i, o in enumerate(oracles)
    ]
