"""Shared by test_grids.py (CPU) and test_gpu_grids.py (MI355X): the rank grids beyond 2 x 2, their numpy references
(computed once and left read-only), a runner of P thread ranks, and a report that says where a wrong board is wrong.

Every case is a global H x W board under ``decomp="2d"``, pattern 5 with seed 17, 40 generations at ``halo_depth=16``
and ``kernel_depth=8``: two supersteps of two passes and a one-pass remainder of 8, so the earlier pass of a superstep
stores ghost rows and ghost words.  What only each case reaches:

    3x3  200 x 448  tiles 66-67 rows x 192/128/128 columns: eight distinct neighbours, uneven h and nw, ranks of three
                    and of two words, a centre rank that touches no edge of a bounded board
    3x3  100 x 192  one-word tiles: the W and the E item send the same word, both ghost words sit next to it
    3x3   20 x 448  tiles of 6-7 rows: the halo depth clamps to 6 and h <= 2k, so no interior / band split
    4x2  150 x 576  Py = 2: N and S are one peer, NW and SW are one peer, E and W are not
    2x4  203 x 320  the grid an 8-rank square board gets; Px = 2: E and W are one peer, N and S are not
    3x1  100 x 448  no y neighbours: W / E items only, no corners, ghost words but no ghost rows
    4x1   64 x 256  the same with one-word tiles
"""
import collections
import functools
import threading
import time

import numpy as np

from gol_amd.ops import numpy_census, numpy_step_rule, numpy_step_rule_bounded, random_board

Case = collections.namedtuple("Case", "grid P H W")

CASES = [
    Case("3x3", 9, 200, 448),
    Case("3x3", 9, 100, 192),
    Case("3x3", 9, 20, 448),
    Case("4x2", 8, 150, 576),
    Case("2x4", 8, 203, 320),
    Case("3x1", 3, 100, 448),
    Case("4x1", 4, 64, 256),
]
CONWAY, HIGHLIFE, B1 = "B3/S23", "B36/S23", "B1/S012345678"
SEED, GENS, HALO, KDEPTH = 17, 40, 16, 8
JOIN_S = 120


def case_id(case):
    return f"{case.grid}-{case.H}x{case.W}"


def pick(*numbers):
    """The cases of the table above by their 1-based row."""
    return [CASES[n - 1] for n in numbers]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def start_board(case):
    return _frozen(random_board(case.H, case.W, SEED))


@functools.lru_cache(maxsize=None)
def reference(case, rule, boundary):
    """``(counts, board)`` of the case after GENS generations: the census oracle's series and its last board, which
    is ``numpy_step_rule`` / ``numpy_step_rule_bounded`` one generation at a time."""
    counts, board = numpy_census(start_board(case), rule, GENS, bounded=boundary == "dead", return_board=True)
    return _frozen(counts), _frozen(board)


def board_after(case, rule, boundary):
    return reference(case, rule, boundary)[1]


def halo_depth_of(case):
    """The depth every rank runs at: the 16 asked for, clamped to the shortest tile (2-D: and to 63)."""
    py = int(case.grid.split("x")[1])
    return min(HALO, case.H // py)


def exchanges_of(case):
    """One exchange per superstep of the clamped depth (init-time timing exchanges are not counted by stats())."""
    return -(-GENS // halo_depth_of(case))


Part = collections.namedtuple("Part", "rank cx cy row0 col0 board stats result")


def run_ranks(gol, case, backend, script=None, **kw):
    """The case on P thread ranks, one daemon thread each, joined within JOIN_S seconds: ``script(sim)`` (default:
    GENS generations) runs after ``init(5, seed=SEED)``.  Returns a Part per rank; ``stats`` is taken after init."""
    hip = backend == "hip"
    ts = gol.parallel.p2p_thread_transports(case.P) if hip else gol.parallel.thread_transports(case.P)
    parts, errs = [None] * case.P, []
    if hip:
        kw.setdefault("device", 0)

    def rank_main(r):
        try:
            s = gol.Simulation(case.H, ts[r], backend=backend, global_mode=True, width=case.W, decomp="2d", grid=case.grid,
                               halo_depth=HALO, kernel_depth=KDEPTH, **kw)
            s.init(5, seed=SEED)
            stats = s.stats()
            result = None
            if script:
                result = script(s)
            else:
                s.step(GENS)
            g = s.geometry
            stats = dict(stats, exchanges=s.stats()["exchanges"])
            parts[r] = Part(r, g.cx, g.cy, g.row0, g.col0, s.board(), stats, result)
        except Exception as e:  # reported below
            errs.append(f"rank {r}: {e!r}")

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(case.P)]
    for t in th:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in th:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(th) if t.is_alive()]
    assert not alive, f"ranks {alive} still running after {JOIN_S} s; errors so far: {errs}"
    assert not errs, errs
    px, py = (int(v) for v in case.grid.split("x"))
    assert sorted((p.cx, p.cy) for p in parts) == sorted((x, y) for x in range(px) for y in range(py))
    return parts


def assemble(case, parts):
    full = np.full((case.H, case.W), 255, np.uint8)  # (a cell no rank owns stays 255 and fails every comparison)
    for p in parts:
        full[p.row0 : p.row0 + p.board.shape[0], p.col0 : p.col0 + p.board.shape[1]] = p.board
    return full


def mismatch_report(parts, got, ref, halo=HALO):
    """Where ``got`` differs from ``ref``, tile by tile: the wrong cells of each rank ``(cx, cy)``, and how many of them
    lie in the tile's first or last ``halo`` rows (what the N / S items feed), in its first or last 64-cell word
    (W / E), and in the four corner blocks where the two meet (NW, NE, SW, SE).  Empty when the boards are equal."""
    bad = np.asarray(got) != np.asarray(ref)
    if not bad.any():
        return ""
    lines = [f"{int(bad.sum())} of {bad.size} cells differ"]
    for p in sorted(parts, key=lambda q: (q.cy, q.cx)):
        h, w = p.board.shape
        t = bad[p.row0 : p.row0 + h, p.col0 : p.col0 + w]
        if not t.any():
            continue
        rows = np.zeros(h, bool)
        rows[: min(halo, h)] = rows[max(0, h - halo) :] = True
        cols = np.zeros(w, bool)
        cols[: min(64, w)] = cols[max(0, w - 64) :] = True
        lines.append(
            f"rank {p.rank} (cx {p.cx}, cy {p.cy}; rows {p.row0}..{p.row0 + h - 1}, columns {p.col0}..{p.col0 + w - 1}): "
            f"{int(t.sum())} wrong, {int(t[rows].sum())} in the first/last {halo} rows, "
            f"{int(t[:, cols].sum())} in the first/last word, {int(t[np.ix_(rows, cols)].sum())} in the corner blocks"
        )
    return "\n".join(lines)


def check_board(case, parts, ref):
    """The assembled global board is ``ref``, bit for bit; the failure message is the mismatch report."""
    got = assemble(case, parts)
    assert np.array_equal(got, ref), mismatch_report(parts, got, ref, halo_depth_of(case))
    return got


def check_census(case, parts, rule, boundary):
    """Every rank holds the oracle's series from generation 1 on, its last count is population(), the series has at
    least two distinct values and the board is exact.  ``parts`` come from ``run_ranks(..., script=census_script)``."""
    counts, board = reference(case, rule, boundary)
    check_board(case, parts, board)
    assert len(set(counts.tolist())) >= 2
    for p in parts:
        start, series, pop = p.result
        assert start == 0, (p.rank, start)
        assert series.dtype == np.uint64 and np.array_equal(series, counts), (p.rank, series.tolist(), counts.tolist())
        assert pop == int(counts[-1]), (p.rank, pop)


def census_script(s):
    s.step(GENS)
    start, series = s.census()
    return start, series, s.population()


# ----- views on the first case: windows, density maps and stamps whose rectangles span four and nine ranks -----

def np_window(board, r0, c0, rows, cols):
    return np.take(np.take(board, np.arange(r0, r0 + rows), axis=0, mode="wrap"), np.arange(c0, c0 + cols), axis=1,
                   mode="wrap")


def np_density(board, br, bc):
    H, W = board.shape
    gh, gw = -(-H // br), -(-W // bc)
    pad = np.zeros((gh * br, gw * bc), np.uint32)
    pad[:H, :W] = board
    return pad.reshape(gh, br, gw, bc).sum(axis=(1, 3)).astype(np.uint32)


def np_stamp(board, pat, r0, c0, mode):
    out = board.copy()
    idx = np.ix_((r0 + np.arange(pat.shape[0])) % board.shape[0], (c0 + np.arange(pat.shape[1])) % board.shape[1])
    cur = out[idx]
    out[idx] = {"or": cur | pat, "replace": pat, "xor": cur ^ pat}[mode]
    return out


VIEW_CASE = CASES[0]
WIN_NINE = (60, 180, 80, 160)   # rows cross 67 and 134, columns cross 192 and 320: all nine ranks contribute
WIN_SEAMS = (190, 440, 20, 20)  # across both torus seams
DENSITIES = [(7, 128), (64, 64)]  # (7, 128): two-word blocks against column starts at words 3 and 5, 7-row blocks
#                                   against row starts 67 and 134 -- blocks straddle ranks in both axes
AT_FOUR, AT_SEAMS = (50, 170), (190, 430)  # the 37 x 70 pattern over four ranks (xor), across the seams (replace)
VIEW_GENS = 9


def view_pattern():
    return (np.random.default_rng(5).random((37, 70)) < 0.4).astype(np.uint8)


def views_script(bounded):
    """The script one simulation runs (on a bounded board only the rectangles inside the board)."""
    H, W = VIEW_CASE.H, VIEW_CASE.W
    pat = view_pattern()

    def script(s):
        res = {"nine": s.window(*WIN_NINE)}
        if not bounded:
            res["seams"] = s.window(*WIN_SEAMS)
        for br, bc in DENSITIES:
            res[f"d{br}x{bc}"] = s.density(br, bc)
        s.stamp(pat, at=AT_FOUR, mode="xor")
        if not bounded:
            s.stamp(pat, at=AT_SEAMS, mode="replace")
        res["stamped"] = s.window(0, 0, H, W)
        s.step(VIEW_GENS)
        res["stepped"] = s.window(0, 0, H, W)
        res["nine_after"] = s.window(*WIN_NINE)
        res["d_after"] = s.density(*DENSITIES[0])
        res["pop"] = np.uint64(s.population())
        return res

    return script


@functools.lru_cache(maxsize=None)
def views_expected(bounded):
    """What views_script returns, from numpy alone."""
    b0, pat = start_board(VIEW_CASE), view_pattern()
    res = {"nine": np_window(b0, *WIN_NINE)}
    if not bounded:
        res["seams"] = np_window(b0, *WIN_SEAMS)
    for br, bc in DENSITIES:
        res[f"d{br}x{bc}"] = np_density(b0, br, bc)
    b1 = np_stamp(b0, pat, *AT_FOUR, "xor")
    if not bounded:
        b1 = np_stamp(b1, pat, *AT_SEAMS, "replace")
    res["stamped"] = b1
    b2 = (numpy_step_rule_bounded if bounded else numpy_step_rule)(b1, CONWAY, VIEW_GENS)
    assert not np.array_equal(b2, (numpy_step_rule if bounded else numpy_step_rule_bounded)(b1, CONWAY, VIEW_GENS))
    res["stepped"] = b2
    res["nine_after"] = np_window(b2, *WIN_NINE)
    res["d_after"] = np_density(b2, *DENSITIES[0])
    res["pop"] = np.uint64(b2.sum())
    return {k: _frozen(np.asarray(v)) for k, v in res.items()}


def check_views(results, expected, who):
    assert set(results) == set(expected), (who, sorted(results), sorted(expected))
    for key, want in expected.items():
        got = np.asarray(results[key])
        assert got.shape == want.shape and np.array_equal(got, want), (
            who, key, int((got != want).sum()) if got.shape == want.shape else (got.shape, want.shape))
