"""Shared cases of the pattern-matching tests (test_match.py: CPU backend; test_gpu_match.py: HIP backend).

Every comparison is exact against ``ops.numpy_match`` (np.roll on the torus, zero padding on the bounded board) applied to
``sim.board()`` or ``batch.boards()``.  One simulation per (backend, board, boundary) is built once and shared; each check
sets the board it needs.
"""
import functools

import numpy as np

from gol_amd.ops import match_template, numpy_match, random_board

SEED = 4242
GLIDER = "x = 3, y = 3, rule = B3/S23\nbob$2bo$3o!"
GLIDER_CELLS = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)
BLOCK = np.ones((2, 2), dtype=np.uint8)
BLINKER = np.ones((1, 3), dtype=np.uint8)
BEEHIVE = np.array([[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0]], dtype=np.uint8)

# rows x cols: one word; word seams; 36 cells in the last word; 2 cells in the last word (the seam funnel takes almost a
# whole word from word 0)
BOARDS = [(64, 64), (128, 192), (96, 100), (70, 130)]
# HIP only: 65 words (a second lane group of one lane); the row stride
HIP_BOARDS = [(64, 4160), (300, 64)]
BOUNDARIES = ["torus", "dead"]


def bid(shape):
    return f"{shape[0]}x{shape[1]}"


_sims = {}


def sim_of(gol, backend, shape, boundary):
    key = (backend, shape, boundary)
    if key not in _sims:
        kw = {"device": 0} if backend == "hip" else {}
        _sims[key] = gol.Simulation(shape[0], width=shape[1], backend=backend, boundary=boundary, **kw).init(0)
    return _sims[key]


@functools.lru_cache(maxsize=None)
def random_cells(shape):
    b = random_board(shape[0], shape[1], SEED)
    b.setflags(write=False)
    return b


def turned(cells, k):
    """Orientation k of a 0/1 array: ids 0..3 clockwise quarter turns, 4..7 the same of the left-right mirror image."""
    a = np.fliplr(cells) if k >= 4 else cells
    return np.ascontiguousarray(np.rot90(a, -(k & 3)))


def stamp_wrapped(board, cells, r0, c0):
    """cells onto board with its first cell at (r0, c0), wrapping (the callers keep bounded stamps inside)."""
    H, W = board.shape
    for (i, j), v in np.ndenumerate(cells):
        if v:
            board[(r0 + i) % H, (c0 + j) % W] = 1


def glider_origins(shape, boundary):
    H, W = shape
    if boundary == "torus":
        # the word seam; the torus seams; the torus corner
        out = [(10, 62 % W), (10, W - 2), (H - 2, 10), (H - 2, W - 2)]
        return sorted(set(out))
    # flush in the four corners (the ring lies off the board) and against the partial last word
    return sorted({(0, 0), (0, W - 3), (H - 3, 0), (H - 3, W - 3), (20, W - 3), (30, 61 if W > 64 else 30)})


def assert_result(res, board, template, boundary, orientations):
    pos, ids = numpy_match(board, template, boundary, orientations)
    assert res.count == len(pos)
    assert not res.truncated
    assert res.positions.dtype == np.int64 and res.positions.shape == (len(pos), 2)
    assert np.array_equal(res.positions, pos)
    assert res.orientation.dtype == np.uint8 and np.array_equal(res.orientation, ids)
    return pos, ids


# ---- 1. placed gliders on an empty board -----------------------------------------------------------------------------

def check_placed_gliders(gol, backend, shape, boundary):
    s = sim_of(gol, backend, shape, boundary)
    origins = glider_origins(shape, boundary)
    board = np.zeros(shape, dtype=np.uint8)
    for r, c in origins:
        stamp_wrapped(board, GLIDER_CELLS, r, c)
    s.set_board(board)
    assert np.array_equal(s.board(), board)
    res = s.match(GLIDER, margin=1)
    t = match_template(GLIDER, 1)
    assert t.shape == (5, 5) and t.ring == 1
    pos, _ = assert_result(res, board, t, boundary, False)
    assert [tuple(p) for p in pos] == origins  # the stamped origins, no other
    assert s.count_matches(GLIDER) == len(origins)
    assert s.count_matches(GLIDER_CELLS) == len(origins)  # (an array is a pattern too)


def check_eight_orientations(gol, backend, shape, boundary):
    H, W = shape
    s = sim_of(gol, backend, shape, boundary)
    board = np.zeros(shape, dtype=np.uint8)
    spots = {}
    for k in range(8):  # two rows of four, one of them across the word seam / against the last word
        r0, c0 = 8 + 24 * (k // 4), (6 + 16 * (k % 4)) if k != 3 else min(62, W - 4)
        if boundary == "torus" and k == 7:
            r0, c0 = H - 2, W - 2  # the torus corner
        stamp_wrapped(board, turned(GLIDER_CELLS, k), r0, c0)
        spots[(r0, c0)] = k
    s.set_board(board)
    res = s.match(GLIDER, orientations="all")
    pos, ids = assert_result(res, board, match_template(GLIDER), boundary, "all")
    assert {tuple(p): int(k) for p, k in zip(pos, ids)} == spots
    assert s.count_matches(GLIDER, orientations="all") == 8
    assert s.count_matches(GLIDER) == 1


# ---- 2. random boards ------------------------------------------------------------------------------------------------

def copied_template(board, boundary, th, tw, ring, care, at):
    """A template whose values are the board's around `at` (so that it matches there)."""
    H, W = board.shape
    value = np.zeros((th, tw), dtype=np.uint8)
    for i in range(th):
        for j in range(tw):
            r, c = at[0] - ring + i, at[1] - ring + j
            if boundary == "torus":
                value[i, j] = board[r % H, c % W]
            elif 0 <= r < H and 0 <= c < W:
                value[i, j] = board[r, c]
    return match_template(value=value * care, care=care, ring=ring)


def sparse_care():
    """40 care cells of a 32 x 32 template, the four corners among them."""
    rng = np.random.default_rng(7)
    care = np.zeros((32, 32), dtype=np.uint8)
    care[0, 0] = care[0, 31] = care[31, 0] = care[31, 31] = 1
    while care.sum() < 40:
        care[rng.integers(32), rng.integers(32)] = 1
    return care


RANDOM_CASES = ["3x3", "1x32", "32x1", "32x32_ring0", "32x32_ring15", "2x2_dead"]


def random_case(name, board, boundary):
    H, W = board.shape
    far = (H - 3, W - 3) if boundary == "torus" else (20, 20)  # (torus: the 32 x 32 box crosses both seams)
    if name == "3x3":
        return copied_template(board, boundary, 3, 3, 1, np.ones((3, 3), np.uint8), (H - 1, W - 1))
    if name == "1x32":
        return copied_template(board, boundary, 1, 32, 0, np.ones((1, 32), np.uint8), (5, W - 7))
    if name == "32x1":
        return copied_template(board, boundary, 32, 1, 0, np.ones((32, 1), np.uint8), (H - 7, 5))
    if name == "32x32_ring0":
        return copied_template(board, boundary, 32, 32, 0, sparse_care(), far)
    if name == "32x32_ring15":
        return copied_template(board, boundary, 32, 32, 15, sparse_care(), far)
    return match_template(value=np.zeros((2, 2), np.uint8), care=np.ones((2, 2), np.uint8), ring=0)


def check_random(gol, backend, shape, boundary):
    s = sim_of(gol, backend, shape, boundary)
    board = random_cells(shape)
    s.set_board(board)
    for name in RANDOM_CASES:
        t = random_case(name, board, boundary)
        pos, _ = numpy_match(board, t, boundary)
        assert len(pos) >= 1, name  # no case is vacuous
        if name == "2x2_dead":  # about 1/16 of the cells, at both column parities
            assert len(pos) > shape[0] * shape[1] // 32 and len({int(c) & 1 for c in pos[:, 1]}) == 2
        assert_result(s.match(t), board, t, boundary, False)
    # every orientation of an asymmetric sparse template
    t = random_case("32x32_ring15", board, boundary)
    assert_result(s.match(t, orientations="all"), board, t, boundary, "all")


# ---- 3. the current board --------------------------------------------------------------------------------------------

def check_current_board(gol, backend, shape, boundary):
    s = sim_of(gol, backend, shape, boundary)
    s.set_board(random_cells(shape))
    s.step(8)
    board = s.board()
    assert not np.array_equal(board, random_cells(shape))
    for pattern in (BLOCK, BLINKER):
        t = match_template(pattern)
        assert_result(s.match(pattern, orientations="all"), board, t, boundary, "all")
    before = s.stats()["match_launches"]
    assert s.count_matches(BLINKER, orientations="all") == len(numpy_match(board, match_template(BLINKER), boundary, "all")[0])
    assert s.stats()["match_launches"] - before == 2  # a blinker has two orientations


# ---- 4. truncation ---------------------------------------------------------------------------------------------------

def check_truncation(gol, backend):
    s = sim_of(gol, backend, (64, 64), "torus")
    s.set_board(np.zeros((64, 64), dtype=np.uint8))
    t = match_template(value=[[0]], care=[[1]], ring=0)
    pos, _ = numpy_match(np.zeros((64, 64), np.uint8), t)
    assert len(pos) == 4096
    res = s.match(t, max_hits=100)
    assert res.count == 4096 and res.truncated
    assert res.positions.shape == (100, 2) and res.orientation.shape == (100,)
    got = [tuple(p) for p in res.positions]
    assert got == sorted(set(got))  # sorted, no duplicate
    assert set(got) <= {tuple(p) for p in pos}
    nopos = s.match(t, max_hits=100, positions=False)
    assert nopos.count == 4096 and nopos.truncated and nopos.positions.shape == (0, 2)
    assert s.count_matches(t) == 4096
    full = s.match(t, max_hits=4096)
    assert full.count == 4096 and not full.truncated and np.array_equal(full.positions, pos)


# ---- 5. tensor output ------------------------------------------------------------------------------------------------

def check_tensor(gol, backend, shape, boundary):
    import torch

    s = sim_of(gol, backend, shape, boundary)
    board = random_cells(shape)
    s.set_board(board)
    # (templates that do occur on a random board: four dead cells, three live cells in a line either way, the sparse one)
    for pattern, orientations in ((random_case("2x2_dead", board, boundary), False), (match_template(BLINKER, 0), "all"),
                                  (random_case("32x32_ring15", board, boundary), "all")):
        t = pattern
        pos, _ = numpy_match(board, t, boundary, orientations)
        want = np.zeros(shape, dtype=np.uint8)
        want[pos[:, 0], pos[:, 1]] = 1
        assert want.any()
        for dtype in (torch.uint8, torch.bool):
            got = s.match_tensor(pattern, orientations=orientations, dtype=dtype)
            assert got.dtype == dtype and tuple(got.shape) == shape
            assert got.is_cuda == (backend == "hip")
            assert np.array_equal(got.cpu().numpy().astype(np.uint8), want)
        out = torch.full(shape, 7, dtype=torch.uint8, device=got.device)
        assert s.match_tensor(pattern, orientations=orientations, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want)
    assert s.match_tensor(BLOCK).dtype == torch.uint8  # the default


# ---- 6. refusals -----------------------------------------------------------------------------------------------------

def check_refusals(gol, backend, pytest):
    s = sim_of(gol, backend, (64, 64), "torus")
    s.set_board(random_cells((64, 64)))
    before = s.stats()["match_launches"]
    ones = np.ones((3, 3), np.uint8)
    with pytest.raises(ValueError, match="33"):  # a shape over 32
        s.match(np.ones((31, 4), np.uint8), margin=1)
    with pytest.raises(ValueError, match="33"):
        match_template(value=np.ones((33, 2), np.uint8), care=np.ones((33, 2), np.uint8))
    with pytest.raises(ValueError, match="no care cell"):
        match_template(value=np.zeros((3, 3), np.uint8), care=np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError, match="outside care"):
        match_template(value=ones, care=np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError, match="ring = 2"):
        match_template(value=np.ones((4, 6), np.uint8), care=np.ones((4, 6), np.uint8), ring=2)
    with pytest.raises(ValueError, match="margin = -1"):
        s.match(GLIDER, margin=-1)
    with pytest.raises(ValueError, match="not 0 or 1"):
        s.match(np.array([[0, 2], [1, 0]]))
    with pytest.raises(ValueError, match="not 0 or 1"):
        match_template(value=ones, care=ones * 3)
    with pytest.raises(ValueError, match="max_hits = 0"):
        s.match(GLIDER, max_hits=0)
    with pytest.raises(ValueError, match="orientations"):
        s.match(GLIDER, orientations="some")
    # th > H: a 20 x 64 board
    kw = {"device": 0} if backend == "hip" else {}
    small = gol.Simulation(20, width=64, backend=backend, **kw).init(0)
    with pytest.raises(ValueError, match="the board 20 x 64"):
        small.match(match_template(value=np.ones((21, 1), np.uint8)))
    with pytest.raises(ValueError, match="the board 20 x 64"):
        small.match_tensor(match_template(value=np.ones((21, 2), np.uint8)))
    with pytest.raises(ValueError, match="the board 20 x 64"):
        small.count_matches(match_template(value=np.ones((1, 21), np.uint8)), orientations="all")  # (turned: 21 rows)
    with pytest.raises(ValueError, match="the board 20"):
        small.engine.match([(0, match_template(value=np.ones((21, 1), np.uint8)).native)], 10, True)  # the native check
    # tw > W needs a board narrower than 32 cells: the check is the backends' common code, run on the CPU backend
    if backend == "cpu":
        narrow = gol.Simulation(40, width=8, backend="cpu").init(0)
        with pytest.raises(ValueError, match="the board 40 x 8"):
            narrow.match(match_template(value=np.ones((1, 9), np.uint8)))
        with pytest.raises(ValueError, match="9 columns, the board 8"):
            narrow.engine.match([(0, match_template(value=np.ones((1, 9), np.uint8)).native)], 10, True)
        assert narrow.stats()["match_launches"] == 0
        assert narrow.count_matches(np.ones((1, 1), np.uint8), margin=0) == 0 and narrow.count_matches([[0]], margin=0) == 320
    with pytest.raises(ValueError, match="max_hits = 0"):
        small.engine.match([(0, match_template(BLOCK).native)], 0, True)
    assert small.stats()["match_launches"] == 0 and s.stats()["match_launches"] == before  # nothing was launched


def check_two_ranks(gol, backend):
    import wide_cases as wc

    def script(s):
        refused = []
        for call in (lambda: s.match(GLIDER), lambda: s.count_matches(BLOCK), lambda: s.match_tensor(BLOCK),
                     lambda: s.engine.match([(0, match_template(BLOCK).native)], 10, True)):
            try:
                call()
                refused.append(None)
            except ValueError as e:
                refused.append(str(e))
        return refused, s.stats()["match_launches"]

    for p in wc.run_ranks(gol, 2, 64, 64, backend, script):
        refused, launches = p.result
        assert all(r is not None and "2 ranks" in r for r in refused), refused
        assert launches == 0


# ---- 7. soup counts --------------------------------------------------------------------------------------------------

SOUP_PATTERNS = [BLOCK, BLINKER, BEEHIVE, GLIDER]
N_RANDOM_SOUPS = 300


def placed_soups():
    """5 soups of 64^2, 3 of 128^2 and 3 of 256^2 with blocks, blinkers, beehives and gliders across the row wrap S - 1 -> 0,
    the column wrap, the word seam 63 | 64 of a 128^2 soup, the word seams 127 | 128 and 191 | 192 of a 256^2 soup (k_match
    with nw = pitch = 4), and the corner."""
    def soups(S, n):
        b = np.zeros((n, S, S), dtype=np.uint8)
        stamp_wrapped(b[0], BLOCK, S - 1, 10)               # across the row wrap
        stamp_wrapped(b[0], BLINKER, 20, S - 1)             # across the column wrap
        stamp_wrapped(b[0], BEEHIVE, 40, 30)
        stamp_wrapped(b[1], BLOCK, S - 1, S - 1)            # the corner
        stamp_wrapped(b[1], turned(GLIDER_CELLS, 2), 10, 10)
        stamp_wrapped(b[1], turned(BLINKER, 1), S - 2, 40)  # vertical, across the row wrap
        stamp_wrapped(b[2], GLIDER_CELLS, S - 2, S - 2)     # a glider on the corner
        stamp_wrapped(b[2], turned(BEEHIVE, 1), S - 2, 20)
        stamp_wrapped(b[2], BLOCK, 30, 30)
        stamp_wrapped(b[2], BLOCK, 30, 33)                  # two blocks one cell apart: neither is isolated
        if S == 128:
            stamp_wrapped(b[0], BLOCK, 50, 63)              # across the word seam
            stamp_wrapped(b[1], BLINKER, 70, 62)
            stamp_wrapped(b[2], BEEHIVE, 90, 62)
            stamp_wrapped(b[2], turned(GLIDER_CELLS, 5), 60, 62)
        if S == 256:  # the four patterns across each of the word seams 127 | 128 and 191 | 192, one soup per seam
            for i, seam in enumerate((128, 192)):
                stamp_wrapped(b[i], BLOCK, 50, seam - 1)
                stamp_wrapped(b[i], BLINKER, 70, seam - 2)
                stamp_wrapped(b[i], BEEHIVE, 90, seam - 2)
                stamp_wrapped(b[i], turned(GLIDER_CELLS, 5 + i), 60, seam - 2)
                stamp_wrapped(b[i], turned(BEEHIVE, 1), 110, seam - 1)
            stamp_wrapped(b[2], BLOCK, 127, 63)             # the crossing of the seams 63 | 64 and rows 127 | 128
            stamp_wrapped(b[0], BLOCK, 150, 255)            # across the column wrap 255 | 0, beside the blinker at row 20
            stamp_wrapped(b[0], GLIDER_CELLS, 200, 254)
            stamp_wrapped(b[1], BEEHIVE, 150, 254)
        for k in range(3, n):
            stamp_wrapped(b[k], turned(GLIDER_CELLS, k), 5 * k, S - 3 + k)
            stamp_wrapped(b[k], BEEHIVE, S - 2, 7 * k)
        return b

    return soups(64, 5), soups(128, 3), soups(256, 3)


def oracle_counts(boards, orientations="all"):
    out = np.zeros((len(boards), len(SOUP_PATTERNS)), dtype=np.uint32)
    for i, b in enumerate(boards):
        for t, p in enumerate(SOUP_PATTERNS):
            out[i, t] = len(numpy_match(b, match_template(p), "torus", orientations)[0])
    return out


_soup_oracle = {}


def check_placed_soups(gol, backend):
    for boards in placed_soups():
        batch = gol.SoupBatch.from_boards(boards, backend=backend)
        key = ("placed", boards.shape)
        if key not in _soup_oracle:
            _soup_oracle[key] = oracle_counts(boards)
        want = _soup_oracle[key]
        assert want[0, 0] >= 1 and want[0, 1] >= 1 and want[0, 2] >= 1 and want[2, 3] >= 1 and want[1, 3] >= 1
        if boards.shape[1] == 256:  # block, blinker, beehive, glider: the oracle finds every stamp of the two seam soups
            assert list(want[0]) == [3, 2, 3, 2] and list(want[1]) == [2, 2, 3, 2]
        got = batch.match_counts(SOUP_PATTERNS)
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(got, want)
        assert np.array_equal(batch.match_counts(SOUP_PATTERNS, orientations=False), oracle_counts(boards, False))
        batch.step(4)  # a pending step() is included
        assert np.array_equal(batch.match_counts(SOUP_PATTERNS), oracle_counts(batch.boards()))


def random_soup_counts(gol, backend):
    """match_counts of the 300 seeded random soups after settle(200) and again after settle(2000), each with the boards it
    was counted on and the periods.  Brent's search has settled no soup of seeds 0..299 by generation 200 (all are
    counted mid-run) and 147 of them by generation 2000 (those stand at the generation of their hit, the rest at 2000)."""
    batch = gol.SoupBatch(N_RANDOM_SOUPS, 64, backend=backend, seed=0)
    out = []
    for gens in (200, 2000):
        rec = batch.settle(gens)
        out.append((batch.match_counts(SOUP_PATTERNS), batch.boards(), rec.period))
    return out


def check_random_soups(gol, backend):
    stages = random_soup_counts(gol, backend)
    settled = int((stages[1][2] != 0).sum())
    assert 0 < settled < N_RANDOM_SOUPS  # the second stage mixes settled and running soups
    for k, (got, boards, _) in enumerate(stages):
        if ("random", k) not in _soup_oracle:
            _soup_oracle["random", k] = (oracle_counts(boards), boards)
        want, ref_boards = _soup_oracle["random", k]
        assert np.array_equal(boards, ref_boards)  # (both backends stand on the same boards)
        assert want.sum(axis=0).min() >= 1
        assert np.array_equal(got, want)
    with_pytest_refusal(gol, backend)


def with_pytest_refusal(gol, backend):
    import pytest

    batch = gol.SoupBatch(2, 64, backend=backend)
    with pytest.raises(ValueError, match="not 0 or 1"):
        batch.match_counts([np.array([[0, 5]])])
    with pytest.raises(ValueError, match="33"):
        batch.match_counts([np.ones((31, 31), np.uint8)])
    with pytest.raises(ValueError, match="margin = -2"):
        batch.match_counts([BLOCK], margin=-2)
