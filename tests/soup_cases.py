"""Shared cases of the soup-batch tests (test_soups.py: CPU backend, oracle, CLI; test_gpu_soups.py: HIP backend).

Every expectation comes from the byte-per-cell oracle ``numpy_soup_settle`` / ``numpy_step_rule``; an oracle result is
computed once per (board, rule) and shared by all tests of both files.  The facts about the random soups (which settle,
by when) were established with the oracle alone; the tests assert them of the oracle before comparing the backend.

At 128^2 and 256^2 dense random soups take tens of thousands of generations, so the boards that settle there come from
three families (below): sparse random boards, the 64^2 soups tiled, and placed boards of period 4 S.  Oracle time on one
CPU core with ``numpy_step_rule`` (0.06 s per 100 generations of 256^2): the slowest case is the sparse 256^2 B3/S23 board,
2.9 s (2049 generations of search, 2 x 1442 + 2 of the transient walk); the 256^2 glider and the 256^2 placed board take
1.8 s each, everything at 128^2 and 64^2 below 1 s, apart from the earlier 128^2 random soups (4.5 s for the two).
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


def cells_board(S, cells):
    b = np.zeros((S, S), dtype=np.uint8)
    for r, c in cells:
        b[r % S, c % S] = 1
    return b


GLIDER = [(1, 2), (2, 3), (3, 1), (3, 2), (3, 3)]  # on the main diagonal, heading down and right
LANE = 37                                           # the lane whose rows the in-wave seam patterns sit on


def patterns(S):
    """The seam patterns of a soup of side S = 64 M, by name.  A lane of the kernel holds rows M l .. M l + M - 1 as M
    words each, so besides the torus seams there are the word seams 64 k - 1 | 64 k (wired inside the lane), the lane
    seams M l - 1 | M l (the DPP ring) and, at M = 4, rows that no other lane ever sees."""
    M = S // 64
    top = M * LANE  # the first row of lane LANE
    board = functools.partial(cells_board, S)
    out = {
        "blinker_rows_seam": board([(S - 1, 10), (0, 10), (1, 10)]),          # vertical, across rows S-1 / 0
        "blinker_cols_seam": board([(20, S - 2), (20, S - 1), (20, 0)]),      # horizontal, across columns S-1 / 0
        "corner_block": board([(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]),
        "empty": board([]),
        "glider": board(GLIDER),
        # vertical, across the lane seam M l - 1 | M l (at M = 1 every row seam is one)
        "blinker_lane_seam": board([(top - 2, 21), (top - 1, 21), (top, 21)]),
    }
    for k in range(1, M):  # horizontal, across the word seam 64 k - 1 | 64 k
        out[f"blinker_word_seam_{k}"] = board([(40, 64 * k - 2), (40, 64 * k - 1), (40, 64 * k)])
    for j in range(M):     # wholly inside word column j: a compare or a store that skips the column sees an empty board
        out[f"blinker_word_{j}"] = board([(50, 64 * j + 30), (50, 64 * j + 31), (50, 64 * j + 32)])
    if M > 1:              # a block on the crossing of the last word seam and a lane seam
        c = 64 * (M - 1)
        out["block_seam_crossing"] = board([(top - 1, c - 1), (top - 1, c), (top, c - 1), (top, c)])
    if M == 4:             # vertical, rows 4 l + 1 .. 4 l + 3: both phases stay inside one lane's rows
        out["blinker_in_lane"] = board([(top + 1, 85), (top + 2, 85), (top + 3, 85)])
    return out


@functools.lru_cache(maxsize=None)
def pattern_oracle(S, name):
    return numpy_soup_settle(patterns(S)[name], "B3/S23", 4 * S * 4, transient=True)


# ---- boards that settle at every size within the oracle's reach: three families -------------------------------------

# Sparse random boards (rng(seed).random((S, S)) < density): (S, rule) -> (density, seed).  Every board is seed 0 of its
# density, and sparse_oracle() asserts the conditions of it; no seed had to be passed over.  (Seeds that would have been:
# 128^2 B3/S23 0.08 seeds 2 and 5 and 256^2 B3/S23 0.08 seed 3 do not settle by the cap.)  Oracle records, for the reader:
# period 2 everywhere; transient / found at 145 / 257, 48 / 65, 915 / 1025, 312 / 513, 1442 / 2049, 365 / 513 in the
# order below.
SPARSE = {
    (64, "B3/S23"): (0.08, 0),
    (64, "B36/S23"): (0.08, 0),
    (128, "B3/S23"): (0.08, 0),
    (128, "B36/S23"): (0.08, 0),
    (256, "B3/S23"): (0.08, 0),
    (256, "B36/S23"): (0.06, 0),
}
SPARSE_FOUND_BY = {64: 2049, 128: 2049, 256: 4097}  # the cap that keeps a case at a few seconds of oracle time
FAMILY_RULES = ["B3/S23", "B36/S23"]
FAMILY_CHUNKS = [(128, "B36/S23"), (256, "B3/S23"), (256, "B36/S23")]  # check_family_chunks: what check_chunks leaves open
SIZES = [64, 128, 256]


@functools.lru_cache(maxsize=None)
def sparse_board(S, rule):
    density, seed = SPARSE[(S, rule)]
    b = (np.random.default_rng(seed).random((S, S)) < density).astype(np.uint8)
    b.setflags(write=False)
    return b


def sparse_conditions(S, oracle):
    """What a sparse board has to show of the oracle alone; the names of the conditions it misses."""
    M = S // 64
    period, transient, generation, _, last = oracle
    missed = []
    if not (period >= 1 and transient >= 1):
        missed.append("settles after a transient")
    if not generation <= SPARSE_FOUND_BY[S]:
        missed.append("found by the cap")
    if not all(last[:, 64 * j:64 * j + 64].any() for j in range(M)):
        missed.append("ash in every word column")
    if not all(last[r::M].any() for r in range(M)):
        missed.append("ash in every in-lane row class")
    return missed


@functools.lru_cache(maxsize=None)
def sparse_oracle(S, rule):
    o = numpy_soup_settle(sparse_board(S, rule), rule, SPARSE_FOUND_BY[S], transient=True)
    assert sparse_conditions(S, o) == [], (S, rule, o[:4])
    return o


def tiled_board(S, seed):
    """The 64^2 random soup ``seed`` tiled to S^2.  On a torus the tiling evolves as the tiling of the 64^2 evolution, so
    the expected record is the 64^2 oracle's with the population times M^2: thousands of dense generations through every
    word and row of the M = 2 and M = 4 kernels at the oracle cost of 64^2.  Its blind spot: all words of a row are equal,
    so a wrong neighbour word or a word left out of the comparison is invisible here; the sparse and placed boards and
    the seam patterns are there for that."""
    M = S // 64
    return np.tile(soup(64, seed), (M, M))


def tiled_oracle(S, rule, seed):
    M = S // 64
    p, t, g, pop, last = settled(64, rule, seed)
    assert p > 0 and t >= 1 and g <= FOUND_BY[(64, rule)]
    return p, t, g, pop * M * M, np.tile(last, (M, M))


@functools.lru_cache(maxsize=None)
def assert_tiling_identity(S, rule, seed, gens=5):
    """The shortcut of tiled_oracle is not taken on trust: a few generations of the oracle at S^2 itself."""
    M = S // 64
    big, small = tiled_board(S, seed), soup(64, seed)
    for _ in range(gens):
        big, small = numpy_step_rule(big, rule, 1), numpy_step_rule(small, rule, 1)
        assert small.any() and np.array_equal(big, np.tile(small, (M, M)))
    return True


T_TETROMINO = [(0, 0), (0, 1), (0, 2), (1, 1)]


def placed_board(S):
    """A glider on the main diagonal (period 4 S: it crosses every row seam and every column seam once per period), a
    T-tetromino (the transient: a traffic light after 9 generations under B3/S23) and a block, both half a board away
    from the glider's track and from each other, the T-tetromino across the word seam 191 | 192 of a 256^2 soup, the
    block on the crossing of a word seam and a lane seam there.  No symmetry."""
    q = S // 4
    cells = list(GLIDER)
    cells += [(q + 1 + r, 3 * q - 1 + c) for r, c in T_TETROMINO]
    cells += [(3 * q - 1 + r, q - 1 + c) for r in (0, 1) for c in (0, 1)]
    return cells_board(S, cells)


@functools.lru_cache(maxsize=None)
def placed_oracle(S, rule):
    """The oracle's own run under each rule (the histories differ: under B36/S23 a dead cell of the T-tetromino's
    generation 8 has six neighbours, and it dies out at 13 instead of becoming a traffic light at 9).  Either way the
    glider sets the period 4 S, and the save at 4 S - 1 is the first on the cycle: found at 8 S - 1."""
    o = numpy_soup_settle(placed_board(S), rule, 16 * S, transient=True)
    transient, population = {"B3/S23": (9, 5 + 12 + 4), "B36/S23": (13, 5 + 4)}[rule]
    assert o[:4] == (4 * S, transient, 8 * S - 1, population), o[:4]
    return o


def short_board(S):
    """A short-lived placed board: the T-tetromino and the block of placed_board without the glider."""
    b = placed_board(S)
    for r, c in GLIDER:
        b[r, c] = 0
    return b


@functools.lru_cache(maxsize=None)
def short_oracle(S, rule):
    o = numpy_soup_settle(short_board(S), rule, 100, transient=True)
    # the save at 15 is the first on the cycle: a traffic light and the block, or the block alone
    assert o[:4] == {"B3/S23": (2, 9, 17, 16), "B36/S23": (1, 13, 16, 4)}[rule]
    return o


def family_case(S, rule, tiles=2):
    """(boards, oracles, names) of a batch mixing the three families; every oracle-only condition is asserted here."""
    boards = [sparse_board(S, rule), placed_board(S)]
    oracles = [sparse_oracle(S, rule), placed_oracle(S, rule)]
    names = ["sparse", "placed"]
    for i in range(tiles):
        assert_tiling_identity(S, rule, SEED + i)
        boards.append(tiled_board(S, SEED + i))
        oracles.append(tiled_oracle(S, rule, SEED + i))
        names.append(f"tiled{i}")
    assert all(o[0] >= 1 and o[1] >= 1 for o in oracles)
    return np.stack(boards), oracles, names


def launches_of(oracles, chunk, transient=True):
    """The launches of one settle(max_gens, transient, chunk) call that settles every soup: the search ends with the last
    hit; the walk of a soup takes period + transient + 1 loop passes (the last one finds the copies equal)."""
    up = lambda a: -(-a // chunk)  # noqa: E731
    return up(max(o[2] for o in oracles)) + (up(max(o[0] + o[1] + 1 for o in oracles)) if transient else 0)


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
    assert o["glider"][:3] == (4 * S, 0, 8 * S - 1)  # the save at 4 S - 1 is on the cycle: found at 511 / 1023 / 2047
    blinkers = [k for k in names if k.startswith("blinker")]
    stills = ["empty", "corner_block"] + [k for k in names if k == "block_seam_crossing"]
    M = S // 64
    assert len(blinkers) == 3 + (M - 1) + M + (M == 4) and len(stills) == 2 + (M > 1)
    assert all(o[k][:4] == (2, 0, 3, 3) for k in blinkers)  # saved at generation 1, hit at 3
    assert all(o[k][:3] == (1, 0, 1) for k in stills)
    sb = gol.SoupBatch.from_boards(np.stack([pats[k] for k in names]), backend=backend)
    res = sb.settle(16 * S, transient=True)
    assert_result(res, sb.boards(), oracles)
    g = names.index("glider")
    assert (res.period[g], res.transient[g], res.generation[g]) == (4 * S, 0, {64: 511, 128: 1023, 256: 2047}[S])
    for k in stills:
        assert (res.period[names.index(k)], res.transient[names.index(k)]) == (1, 0)
    for k in blinkers:
        assert (res.period[names.index(k)], res.generation[names.index(k)]) == (2, 3), k


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


def chunks_and_resumption(make, oracles):
    """Chunks 1, 7 and 4096 and a run resumed twice give the oracles' records and boards (make(): a fresh batch)."""
    for chunk in (1, 7, 4096):
        sb = make()
        assert_result(sb.settle(MAX_GENS, transient=True, chunk=chunk), sb.boards(), oracles)
        assert sb.stats()["launches"] == launches_of(oracles, chunk)
    sb = make()
    first = sb.settle(100)
    assert (first.generation <= 100).all() and (first.transient == -1).all()
    sb.settle(1000, transient=True)
    assert_result(sb.settle(MAX_GENS, transient=True), sb.boards(), oracles)


def check_chunks(gol, backend, S, rule, n):
    oracles = settling_oracles(S, rule, n)
    chunks_and_resumption(lambda: gol.SoupBatch(n, S, rule, backend=backend, seed=SEED), oracles)


def check_family_chunks(gol, backend, S, rule):
    """check_chunks over the three families: saved, tmp and init travel between launches at M * M words per lane, in
    settle and in transient mode.  With the short board in the batch, the resumed run's first call (to 100) settles one
    soup and leaves the others unsettled, the second (to 1000) walks its transient, the third settles the rest."""
    boards, oracles, _ = family_case(S, rule)
    boards, oracles = np.concatenate([boards, short_board(S)[None]]), oracles + [short_oracle(S, rule)]
    assert sorted(o[2] for o in oracles)[0] < 100 < sorted(o[2] for o in oracles)[1] and max(o[2] for o in oracles) > 1000
    chunks_and_resumption(lambda: gol.SoupBatch.from_boards(boards, rule, backend=backend), oracles)


def check_variant(gol, backend, S, rule, chunk=200):
    """One settle(max_gens, transient=True) of a batch mixing the three families: the search's hit and, since every walk
    is longer than the chunk, kSoupTransientDone after a resumed launch, in the (M, GENERIC) pair of (S, rule)."""
    boards, oracles, names = family_case(S, rule)
    n = len(names)
    assert all(o[0] + o[1] + 1 > chunk for o, k in zip(oracles, names) if k != "sparse")  # these walks are resumed
    sb = gol.SoupBatch.from_boards(boards, rule, backend=backend)
    res = sb.settle(MAX_GENS, transient=True, chunk=chunk)
    assert_result(res, sb.boards(), oracles)
    assert sb.stats()["settled"] == n and (res.period > 0).all() and (res.transient >= 0).all()
    assert sb.stats()["kernel"] == f"soups@{S}" + ("" if rule == "B3/S23" else ":rule")
    assert sb.stats()["launches"] == launches_of(oracles, chunk)
    t = sb.boards_tensor()
    assert t.is_cuda == (backend == "hip") and tuple(t.shape) == (n, S, S)
    assert np.array_equal(t.cpu().numpy(), sb.boards())
    return sb


def check_mixed(gol, backend, chunk=512, S=64):
    """Empty boards, gliders and soups interleaved: waves of one launch end at generations 1, 8 S - 1 and in between or
    later, over several launches (at 64^2 the random soups; at the larger sizes the short board, found at 17, the sparse
    board and a tiled one)."""
    pats = patterns(S)
    boards, oracles = [], []
    if S == 64:
        others = [(soup(S, SEED + i), settled(S, "B3/S23", SEED + i)) for i in range(3)]
    else:
        assert_tiling_identity(S, "B3/S23", SEED)
        others = [(short_board(S), short_oracle(S, "B3/S23")), (sparse_board(S, "B3/S23"), sparse_oracle(S, "B3/S23")),
                  (tiled_board(S, SEED), tiled_oracle(S, "B3/S23", SEED))]
    for b, o in others:
        boards += [pats["empty"], pats["glider"], b]
        oracles += [pattern_oracle(S, "empty"), pattern_oracle(S, "glider"), o]
    found = sorted({o[2] for o in oracles})
    assert found[0] == 1 and 8 * S - 1 in found and len(found) >= 3 and found[-1] > chunk
    sb = gol.SoupBatch.from_boards(np.stack(boards), backend=backend)
    res = sb.settle(MAX_GENS, transient=True, chunk=chunk)
    assert_result(res, sb.boards(), oracles)
    assert sb.stats()["launches"] > 1 and sb.stats()["settled"] == len(boards)
    return sb


def check_max_gens_edge(gol, backend, board, oracle, rule="B3/S23"):
    """max_gens one short of the hit leaves the soup unsettled at max_gens; max_gens on the hit finds it, in a resumed
    call and in a fresh one cut into chunks of 7 (never past max_gens: left = max_gens - g)."""
    period, transient, found, pop, last = oracle
    assert period > 0 and found > 1
    sb = gol.SoupBatch.from_boards(board[None], rule, backend=backend)
    res = sb.settle(found - 1)
    assert (res.period[0], res.transient[0], res.generation[0]) == (0, -1, found - 1)
    before = numpy_step_rule(board, rule, found - 1)
    assert np.array_equal(sb.boards()[0], before) and res.population[0] == int(before.sum())
    assert sb.stats()["settled"] == 0
    res = sb.settle(found)
    assert (res.period[0], res.transient[0], res.generation[0], res.population[0]) == (period, -1, found, pop)
    assert np.array_equal(sb.boards()[0], last) and sb.stats()["settled"] == 1
    fresh = gol.SoupBatch.from_boards(board[None], rule, backend=backend)
    assert_result(fresh.settle(found, transient=True, chunk=7), fresh.boards(), [oracle])


def check_max_gens_edges(gol, backend):
    """The 64^2 glider (settle(510): period 0 at 510; settle(511): period 256 at 511) and the short board at 256^2."""
    assert pattern_oracle(64, "glider")[:3] == (256, 0, 511)
    check_max_gens_edge(gol, backend, patterns(64)["glider"], pattern_oracle(64, "glider"))
    for rule in FAMILY_RULES:
        check_max_gens_edge(gol, backend, short_board(256), short_oracle(256, rule), rule)


def csv_lines(oracles):
    return ["soup,period,transient,generation,population"] + [
        f"{i},{o[0]},{o[1]},{o[2]},{o[3]}" for i, o in enumerate(oracles)
    ]
