"""Shared by test_wide_plans.py (CPU) and test_gpu_wide.py (MI355X): boards wide enough for full-width segments.

The planner (plan.cpp pack_waves) cuts a row band into segments of at most 62 words, so a board below 3968 columns
has no full-width segment at all.  The shapes here are the smallest that give each plan feature of the wide,
benchmarked boards; test_wide_plans.py asserts from the lane descriptors that they do:

    64 x 3968  nw 62   every band is exactly one full-width segment; the torus x-wrap sits in lanes 0 / 63, on a
                       bounded board both halo lanes stream ghost words
    64 x 3950  nw 62   unaligned: the tail word (46 cells) is lane 62 of a full-width segment; ghost words on the torus
    64 x 4096  nw 64   62 + 2: full-width waves and packed 4-lane remainders
    70 x 4000  nw 63   62 + 1: the masked tail word (32 cells) is a one-word segment
    50 x 3969  nw 63   the tail word has one valid cell
    48 x 8000  nw 125  62 + 62 + 1: a seam between two full-width segments
    40 x 7936  nw 124  two full-width segments, no remainder, the x-wrap across two waves

Also here: the loop-tail boards (two bands of every height mod 6, one 300-row band pair), the numpy references
(computed once per board, rule and boundary, left read-only), the plan reader, a runner of thread ranks and a report
that says where a wrong board is wrong in terms of the plan: segment, lane, first / last K rows of the band.
"""
import collections
import functools
import threading
import time

import numpy as np

from gol_amd.ops import numpy_census, random_board

SEG = 62  # output words of a full-width segment (plan.hpp kSegWords)
LANES = 64
LANE_STORE = 1
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8]
CONWAY, HIGHLIFE, REPLICATOR, B1 = "B3/S23", "B36/S23", "B1357/S1357", "B1/S012345678"
# B1 puts births just outside every edge of a bounded board at every level of a pass
RULES = {"torus": [HIGHLIFE, REPLICATOR], "dead": [HIGHLIFE, B1]}
BOUNDARIES = ["torus", "dead"]
SEED = 17
SWEEP_GENS = 2 * max(DEPTHS) + 1
JOIN_S = 120

Shape = collections.namedtuple("Shape", "H W full_per_band rest tail_cells")
# full_per_band: full-width segments of one row band; rest: words of the row's remainder segment (0: none);
# tail_cells: valid cells of the last word
SHAPES = [
    Shape(64, 3968, 1, 0, 64),
    Shape(64, 3950, 1, 0, 46),
    Shape(64, 4096, 1, 2, 64),
    Shape(70, 4000, 1, 1, 32),
    Shape(50, 3969, 1, 1, 1),
    Shape(48, 8000, 2, 1, 64),
    Shape(40, 7936, 2, 0, 64),
]
S3968, S3950, S4096, S4000, S3969, S8000, S7936 = SHAPES

# Loop tails: two bands of 21/20, 23/22 and 25/24 rows (rows_per_wave = (H + 1) // 2) are every residue of nrows
# mod 6, and so of the kernels' n = nrows + 2K for every K; the second band has row0 > 0 and ends at the bottom edge.
TAIL_W = 4096
TAIL_HEIGHTS = [41, 45, 49]
TALL = Shape(600, 4096, 1, 2, 64)
TALL_ROWS, TALL_DEPTHS, TALL_GENS = 300, [3, 6, 8], 17


def tail_shape(H):
    return Shape(H, TAIL_W, 1, 2, 64)


def tail_rows(H):
    return (H + 1) // 2


def shape_id(s):
    return f"{s.H}x{s.W}"


def nwords(W):
    return -(-W // 64)


# ----- numpy references -----

def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def start_board(H, W, seed=SEED):
    return _frozen(random_board(H, W, seed))


@functools.lru_cache(maxsize=None)
def history(H, W, rule, boundary, gens=SWEEP_GENS, seed=SEED):
    """``(counts, boards)``: numpy_census's series over ``gens`` generations of the H x W board, and the boards after
    every odd generation and after the last.  One generation of numpy_step_rule / numpy_step_rule_bounded at a time."""
    b = start_board(H, W, seed)
    counts, boards = [], {}
    for g in range(1, gens + 1):
        c, b = numpy_census(b, rule, 1, bounded=boundary == "dead", return_board=True)
        counts.append(int(c[0]))
        if g % 2 or g == gens:
            boards[g] = _frozen(b)
    return _frozen(np.array(counts, np.uint64)), boards


def board_after(s, rule, boundary, gens, total=SWEEP_GENS):
    """The board after ``gens`` generations, from the history over ``total`` (shared by the depths of a sweep)."""
    return history(s.H, s.W, rule, boundary, total)[1][gens]


def counts_until(s, rule, boundary, gens, total=SWEEP_GENS):
    return history(s.H, s.W, rule, boundary, total)[0][:gens]


def told_apart(s, gens, total=SWEEP_GENS):
    """The bounded HighLife reference differs from the torus one (running the torus could not pass)."""
    return not np.array_equal(board_after(s, HIGHLIFE, "dead", gens, total), board_after(s, HIGHLIFE, "torus", gens, total))


# ----- plans -----

Wave = collections.namedtuple("Wave", "index row0 col store nrows")  # row0, col, store: arrays over the 64 lanes


def engine_rows(H, K, rows_per_wave=0):
    """The segment height the HIP engine plans a one-round pass of depth K with (engine_hip_plan.hip): rows_per_wave
    when given, else the shortest the planner allows, 2K rows (every board here fits one round of resident waves)."""
    return rows_per_wave if rows_per_wave > 0 else min(2 * K, H)


def xwrap(W, boundary):
    """Engine::xwrap_by_plan of a rank that is its own x neighbour."""
    return W % 64 == 0 and boundary == "torus"


def build(gol, H, W, K, boundary="torus", rows_per_wave=0, region=None, x_wrap=None):
    """The plan of a pass of depth K over ``region`` (default: the whole tile, rows [0, H) x words [0, nw)) as the
    engine builds it: ``(waves, stats)``, the waves with nrows > 0 only; ``stats["waves"]`` counts the padding too.
    ``x_wrap``: the plan's x-wrap when it is not ``xwrap(W, boundary)`` (False on a rank with x neighbours)."""
    nw = nwords(W)
    region = region if region is not None else (0, H, 0, nw)
    rows = engine_rows(region[1] - region[0], K, rows_per_wave)
    x_wrap = xwrap(W, boundary) if x_wrap is None else x_wrap
    lanes, stats = gol.native.build_plan([tuple(int(v) for v in region)], nw, H, rows, K, x_wrap, False)
    lanes = np.asarray(lanes).reshape(-1, LANES, 4)
    assert stats["waves"] == lanes.shape[0]
    waves = []
    for i, w in enumerate(lanes):
        assert len(set(w[:, 3].tolist())) == 1, f"wave {i}: nrows differs between lanes"
        if w[0, 3] > 0:
            waves.append(Wave(i, w[:, 0].copy(), w[:, 1].copy(), (w[:, 2] & LANE_STORE) != 0, int(w[0, 3])))
    return waves, stats


def is_full_width(w):
    """All 64 lanes stream one row band: one row0 (the issue's definition), and it is one 62-word segment."""
    return len(set(w.row0.tolist())) == 1 and int(w.store.sum()) == SEG and bool(w.store[1:63].all())


def is_packed(w):
    return len(set(w.row0.tolist())) >= 2


def segments(w):
    """The segments of a wave as ``(row0, first word, words)``: maximal runs of store lanes."""
    out, l = [], 0
    while l < LANES:
        if w.store[l]:
            a = l
            while l < LANES and w.store[l] and w.row0[l] == w.row0[a] and w.col[l] == w.col[a] + (l - a):
                l += 1
            out.append((int(w.row0[a]), int(w.col[a]), l - a))
        else:
            l += 1
    return out


def bands_of(waves):
    """The row bands of a plan, ``[(row0, nrows)]`` sorted."""
    return sorted({(r0, w.nrows) for w in waves for r0, _, _ in segments(w)})


def covers_once(waves, region):
    """Every word of ``region`` (r0, r1, c0, c1) is stored by exactly one lane."""
    r0, r1, c0, c1 = region
    n = np.zeros((r1 - r0, c1 - c0), np.int32)
    for w in waves:
        for sr, sc, sn in segments(w):
            n[sr - r0 : sr - r0 + w.nrows, sc - c0 : sc - c0 + sn] += 1
    return bool((n == 1).all())


# ----- where a wrong board is wrong -----

def equal_rows_bands(H, rows):
    """pack_waves's row bands of H rows cut at ``rows`` per band."""
    nch = -(-H // max(1, rows))
    base, extra = divmod(H, nch)
    out, r = [], 0
    for ch in range(nch):
        nr = base + (1 if ch < extra else 0)
        out.append((r, nr))
        r += nr
    return out


def mismatch_report(got, ref, K, bands, row_origin=0, word_origin=0):
    """Where ``got`` differs from ``ref`` (arrays of cells), in terms of the plan: the number of wrong cells, the first
    wrong row and word column, that word's segment (``word // 62``) and its lane in the segment, whether the row lies in
    the first or last K rows of its band (``bands``: ``[(row0, nrows)]`` in tile rows; the arrays' row 0 is tile row
    ``-row_origin`` and their word 0 is tile word ``-word_origin``), and how the wrong cells spread over segments and
    band edges.  Empty when the boards are equal."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return f"shapes differ: {got.shape} against {ref.shape}"
    bad = got != ref
    if not bad.any():
        return ""
    rows, cols = np.nonzero(bad)
    words = cols // 64 - word_origin
    trow = rows - row_origin

    def band_of(r):
        for b0, n in bands:
            if b0 <= r < b0 + n:
                return b0, n
        return None

    def at_edge(r):
        b = band_of(r)
        return b is not None and (r - b[0] < K or b[0] + b[1] - r <= K)

    def edge(r):
        b = band_of(r)
        if b is None:
            return "outside every band"
        where = [f"{name} {K}" for name, hit in (("first", r - b[0] < K), ("last", b[0] + b[1] - r <= K)) if hit]
        return f"band rows {b[0]}..{b[0] + b[1] - 1}, " + ("in its " + " and ".join(where) + " rows" if where else "inside")

    r, w = int(trow[0]), int(words[0])
    lines = [
        f"{int(bad.sum())} of {bad.size} cells differ",
        f"first wrong cell: row {r}, column {int(cols[0])} = word {w}, segment {w // SEG}, lane {w % SEG + 1} of its "
        f"segment; {edge(r)}",
    ]
    segs = collections.Counter((words // SEG).tolist())
    lines.append("wrong cells per segment: " + ", ".join(f"{s}: {n}" for s, n in sorted(segs.items())))
    lanes = collections.Counter((words % SEG + 1).tolist())
    lines.append("lanes hit: " + ", ".join(f"{l}: {n}" for l, n in sorted(lanes.items())[:8]) +
                 (" ..." if len(lanes) > 8 else ""))
    wrong_rows = sorted(set(trow.tolist()))
    lines.append(f"{len(wrong_rows)} wrong rows, {sum(at_edge(x) for x in wrong_rows)} of them in the first / last {K} "
                 f"rows of a band")
    return "\n".join(lines)


def check_board(got, ref, K, bands, **origin):
    assert np.array_equal(got, ref), mismatch_report(got, ref, K, bands, **origin)


def check_census(sim, counts, board, K, bands):
    """The whole series is numpy_census's, the final board is right, the last count is population() and the series
    holds two distinct values."""
    start, got = sim.census()
    assert start == 0 and got.dtype == np.uint64
    check_board(sim.board(), board, K, bands)
    assert np.array_equal(got, counts), (got.tolist(), np.asarray(counts).tolist())
    assert int(got[-1]) == sim.population()
    assert len(set(got.tolist())) >= 2


# ----- thread ranks -----

Part = collections.namedtuple("Part", "rank row0 col0 board stats result")
RANK_GENS, RANK_HALO, RANK_KDEPTH = 40, 16, 8


def run_ranks(gol, P, H, W, backend, script=None, halo_depth=RANK_HALO, kernel_depth=RANK_KDEPTH, **kw):
    """A global H x W board on P thread ranks, one daemon thread each, joined within JOIN_S seconds: ``script(sim)``
    (default: RANK_GENS generations) runs after ``init(5, seed=SEED)``.  A rank that raises fails the test with its
    message; nothing is retried.  ``stats`` is taken after init."""
    hip = backend == "hip"
    ts = gol.parallel.p2p_thread_transports(P) if hip else gol.parallel.thread_transports(P)
    parts, errs = [None] * P, []
    if hip:
        kw.setdefault("device", 0)
    else:
        kw.pop("schedule", None)

    def rank_main(r):
        try:
            s = gol.Simulation(H, ts[r], backend=backend, global_mode=True, width=W, halo_depth=halo_depth,
                               kernel_depth=kernel_depth, **kw)
            s.init(5, seed=SEED)
            stats = s.stats()
            result = None
            if script:
                result = script(s)
            else:
                s.step(RANK_GENS)
            g = s.geometry
            parts[r] = Part(r, g.row0, g.col0, s.board(), stats, result)
        except Exception as e:  # reported below
            errs.append(f"rank {r}: {e!r}")

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in th:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(th) if t.is_alive()]
    assert not alive, f"ranks {alive} still running after {JOIN_S} s; errors so far: {errs}"
    assert not errs, errs
    return parts


def assemble(H, W, parts):
    full = np.full((H, W), 255, np.uint8)  # (a cell no rank owns stays 255 and fails every comparison)
    for p in parts:
        full[p.row0 : p.row0 + p.board.shape[0], p.col0 : p.col0 + p.board.shape[1]] = p.board
    return full


def census_script(s):
    s.step(RANK_GENS)
    start, series = s.census()
    return start, series, s.population()


def check_ranks(H, W, parts, ref, bands, K=RANK_KDEPTH):
    """The assembled board is ``ref``; the failure message is the report of the first wrong rank's tile, in its own
    rows and words (``bands``: the rank plans' row bands in tile rows; ``K``: the pass depth)."""
    got = assemble(H, W, parts)
    if np.array_equal(got, ref):
        return got
    for p in parts:
        h, w = p.board.shape
        rep = mismatch_report(p.board, ref[p.row0 : p.row0 + h, p.col0 : p.col0 + w], K, bands)
        if rep:
            raise AssertionError(f"rank {p.rank} (rows {p.row0}.., columns {p.col0}..):\n{rep}")
    raise AssertionError("cells that no rank owns")
