"""Shared by test_resident_plans.py (CPU) and test_gpu_resident_variants.py (MI355X): step_resident<NW, B>
(csrc/src/hip/resident_kernel.hip) in every variant the planner can pick -- NW in {8, 16} waves per tile, each wave a
band of B rows of the tile's T = nrows + 2 K extended rows.

Here, with no GPU needed:

  * a mirror of ``HipEngine::res_plan`` (engine_hip_resident.hip) under the test knob ``GOL_RESIDENT=tiles,nw``: the
    tile height from ``balanced_rows_per_chunk`` and the tiles from ``build_plan`` through the bindings, the fit tests
    and ``resident_band_rows`` in Python; it predicts the ``resident@K(<tiles> tiles x <nw> waves x <B> rows)`` string
    of stats()["kernel"] (``<tiles>`` counts the padding tiles too: plans are padded to blocks of four);
  * a mirror of ``res_launch``'s cut of G generations into an odd number S of supersteps of at most ``kin``
    generations, and of the kernel's ``active`` predicate (the trapezoid);
  * the table of reachable (NW, B), from the planner's arithmetic alone;
  * the case lists, each board found by a search over the mirror and checked again in test_resident_plans.py;
  * the numpy references (wide_cases.start_board stepped by numpy_step, kept per board).

What the knob can and cannot plan.  ``balanced_rows_per_chunk`` counts a plan in whole blocks of four waves, so for
``tiles`` < 4 no height "fits" and it returns the whole board as one band: ``tiles`` = 1 .. 3 give one tile per
62-word segment of a row, ``tiles`` = 4 .. 7 give up to four tiles, and so on.  Two tiles one above the other are
therefore not plannable; the two-tile plan here is a 64 x 7936 board, whose tiles are each other's neighbour on both
sides in x and their own in y, and the four-tile plans have every tile between two others in y.

The two-tiles-per-CU branch (``per_cu = 2``: tiles of at most 64 extended rows) is reachable for the same reason:
with ``tiles`` = 2 or 3 the one-per-CU round is the whole board as one band, which fails once H + 2 K > 128, while
the second round asks for at least four waves and gets short tiles.  ``two_per_cu_case`` searches for such boards."""
import collections
import functools

import numpy as np

import wide_cases as wc
from gol_amd.ops import numpy_step

CUS = 256                 # the knob clamps ``tiles`` to the card's CUs; every case here asks for far fewer
DEPTHS = [8, 12, 16, 24]  # kernel_depth of the resident kernel (engine_hip_tune.hip)
WAVES = [8, 16]
BANDS = [2, 3, 4, 5, 6, 8, 10, 12, 16]  # resident_band_rows
CAP = {1: 128, 2: 64}     # extended rows of a tile at one / two tiles per CU
FULL_W = 3968             # one full-width segment per band: a tile per band, nothing packed
MIN_H = 64                # resident_eligible()


def ceil_div(a, b):
    return -(-a // b)


def band_rows(n):
    """resident_band_rows: the supported band height >= n, 0 when there is none."""
    return next((b for b in BANDS if b >= n), 0)


def prev_band(B):
    i = BANDS.index(B)
    return BANDS[i - 1] if i else 0


def vid(v):
    return f"{v[0]}x{v[1]}"


@functools.lru_cache(maxsize=None)
def reachable():
    """Every (nw, B) some tile height and depth plans: T = nrows + 2 kin <= the cap, B = band_rows(ceil(T / nw))."""
    out = set()
    for nw in WAVES:
        for per_cu, cap in CAP.items():
            for kin in DEPTHS:
                for nrows in range(1, cap - 2 * kin + 1):
                    B = band_rows(ceil_div(nrows + 2 * kin, nw))
                    if 0 < B <= cap // nw:
                        out.add((nw, B))
    return tuple(sorted(out, key=lambda v: (-v[0], v[1])))


VARIANTS = reachable()


# ----- the mirror of res_plan() -----

Plan = collections.namedtuple("Plan", "per_cu rows B tiles live heights T waves")
# rows: balanced_rows_per_chunk's height; tiles: with the padding; live: tiles with rows; heights: the distinct
# nrows, descending; T: the tallest tile's extended rows at K = kin; waves: wide_cases.Wave of the live tiles


def _native():
    import gol_amd

    return gol_amd


@functools.lru_cache(maxsize=None)
def plan(H, W, kin, tiles, nw):
    """What res_plan(kin) chooses for an H x W torus under GOL_RESIDENT=tiles,nw, or None when nothing fits.
    (resident_blocks_per_cu, an occupancy query, is taken to allow two tiles per CU: the GPU tests assert the string
    this predicts.)"""
    gol = _native()
    words = W // 64
    assert W % 64 == 0 and H >= MIN_H and tiles >= 1 and nw in WAVES
    cus = min(tiles, CUS)
    region = [(0, H, 0, words)]
    for per_cu in (1, 2):
        bmax = CAP[per_cu] // nw
        rows = gol.native.balanced_rows_per_chunk(region, words, H, kin, per_cu * cus, 1, True)
        if rows + 2 * kin > nw * bmax:
            continue
        B = band_rows(ceil_div(rows + 2 * kin, nw))
        if B <= 0 or B > bmax:
            continue
        waves, st = wc.build(gol, H, W, kin, "torus", rows)
        if len(waves) > per_cu * cus:
            continue
        tallest = max(w.nrows for w in waves)
        if tallest + 2 * kin > nw * B:
            continue
        heights = tuple(sorted({w.nrows for w in waves}, reverse=True))
        return Plan(per_cu, rows, B, st["waves"], len(waves), heights, tallest + 2 * kin, tuple(waves))
    return None


def kernel_name(kin, p, nw):
    return f"resident@{kin}({p.tiles} tiles x {nw} waves x {p.B} rows)"


# ----- the mirror of res_launch() and of the kernel's trapezoid -----

Cut = collections.namedtuple("Cut", "S kmax ks")


def cut(G, kin):
    """G generations in one launch: S = ceil(G / kin) supersteps made odd, the first G % S one generation longer."""
    S = ceil_div(G, kin)
    S += S % 2 == 0
    return Cut(S, ceil_div(G, S), tuple(G // S + (s <= G % S) for s in range(1, S + 1)))


def active(b0, B, g, T):
    """The band of rows [b0, b0 + B) computes generation g (1-based) of a superstep of a tile of T extended rows."""
    return b0 + B > g - 1 and b0 < T - g + 1


def empty_waves(nw, B, T):
    """Waves with no row of the tile at all: they only keep the barriers."""
    return [w for w in range(nw) if w * B >= T]


def inactive(nw, B, g, T):
    return [w for w in range(nw) if not active(w * B, B, g, T)]


def halo_reach(p, H, K):
    """The most tiles a tile's K halo rows above it pass through (itself included when the halo wraps round to it)."""
    bands = wc.bands_of(p.waves)
    owner = np.empty(H, np.int64)
    for i, (r0, n) in enumerate(bands):
        owner[r0 : r0 + n] = i
    return max(len({int(owner[(r0 - j) % H]) for j in range(1, K + 1)}) for r0, _ in bands)


# ----- the cases -----

Case = collections.namedtuple("Case", "H W kin tiles nw B")


def case_id(c):
    return f"{c.nw}x{c.B}-{c.H}x{c.W}-k{c.kin}-t{c.tiles}"


def make(H, W, kin, tiles, nw):
    p = plan(H, W, kin, tiles, nw)
    return Case(H, W, kin, tiles, nw, p.B) if p else None


KNOBS = [1, 4, 8, 16, 32, 64]  # ``tiles``: bands of a full-width board (1: the whole board)


def banded(nw, B, nrows_ok, two_heights=False, prefer_deep=True):
    """The smallest FULL_W board of equal bands (or, ``two_heights``, bands of nrows and nrows - 1) that plans (nw, B)
    with a tallest tile of ``nrows`` rows for which ``nrows_ok(nrows, kin)`` holds; None when there is none."""
    best = None
    for kin in DEPTHS:
        for T in range(nw * prev_band(B) + 1, nw * B + 1):
            nrows = T - 2 * kin
            if nrows < 1 or not nrows_ok(nrows, kin):
                continue
            for n in KNOBS:
                H = n * nrows - (1 if two_heights else 0)
                if H < MIN_H or (two_heights and (n == 1 or nrows < 2)):
                    continue
                key = (H, -kin if prefer_deep else kin)
                if best is None or key < best[0]:
                    best = (key, (H, FULL_W, kin, n, nw))
                break
    if best is None:
        return None
    c = make(*best[1])
    assert c is not None and c.B == B, (best, c)
    return c


@functools.lru_cache(maxsize=None)
def fill_case(nw, B):
    """The tallest tile has T = nw x B exactly: the top wave's last register row is the last extended row."""
    c = banded(nw, B, lambda nrows, k: nrows + 2 * k == nw * B)
    assert c is not None, (nw, B)
    return c


@functools.lru_cache(maxsize=None)
def least_case(nw, B):
    """The smallest T that still plans this B, nw x (the band height below) + 1 or 2 x 8 + 1: whole waves are empty."""
    least = max(nw * prev_band(B) + 1, 2 * DEPTHS[0] + 1)
    c = banded(nw, B, lambda nrows, k: nrows + 2 * k == least)
    assert c is not None, (nw, B)
    return c


SHAPES = {
    "one_row": lambda nrows, k: nrows == 1,            # the halo spans K tiles above and below
    "short": lambda nrows, k: 1 < nrows < k,           # ... several tiles
    "tall": lambda nrows, k: nrows >= 2 * k,           # more own rows than halo rows
}


@functools.lru_cache(maxsize=None)
def shape_cases():
    """Per tile shape the variants that can have it, each with its smallest board: ``[(shape, Case)]``."""
    out = []
    for v in VARIANTS:
        for name, ok in SHAPES.items():
            c = banded(*v, ok)
            if c:
                out.append((name, c))
        c = banded(*v, lambda nrows, k: True, two_heights=True)
        if c:
            out.append(("two_heights", c))
    for nw in WAVES:
        out.append(("alone", make(64, 64, 24, 1, nw)))       # one tile, T = 112 > H: it reloads its own rows
        out.append(("pair", make(64, 7936, 8, 2, nw)))       # two tiles side by side
        out.append(("ring4", make(64, 7936, 24, 4, nw)))     # 2 x 2 tiles: every tile has both neighbours in y
    assert all(c is not None for _, c in out)
    return tuple(out)


# superstep cuts: boards of four 3968-column bands that plan 16 x 4 and 8 x 8 alike (T in 49 .. 64) at every depth
CUT_VARIANTS = [(16, 4), (8, 8)]
CUT_ROWS = {8: 40, 12: 32, 16: 24, 24: 16}


def cut_case(nw, kin):
    return make(4 * CUT_ROWS[kin], FULL_W, kin, 4, nw)


def cut_gens(kin):
    return [1, 2, kin - 1, kin, kin + 1, 2 * kin, 2 * kin + 1, 3 * kin + 1]


# widths: what a row is cut into (62-word segments, remainders packed several to a tile)
WIDTHS = [64, 128, 3968, 4032, 4096, 7936]
WIDTH_VARIANTS = [(16, 4), (8, 8)]
WIDTH_KIN = 16


@functools.lru_cache(maxsize=None)
def width_case(W, nw):
    """At 3968 columns and wider the smallest board of four (7936: 2 x 2) tiles that plans WIDTH_VARIANTS' band
    height at depth 16.  At 64 and 128 columns a tile holds many short segments instead (that is the point), so the
    band height is what 96 rows in at most four tiles come to."""
    target = dict(WIDTH_VARIANTS)[nw]
    if W < FULL_W:
        return make(96, W, WIDTH_KIN, 4, nw)
    for H in range(MIN_H, 161):
        c = make(H, W, WIDTH_KIN, 4, nw)
        if c and c.B == target:
            return c
    raise AssertionError((W, nw))


# launch sequences: one simulation stepped (kin, 1, 2 kin + 1, kin - 1, 3 kin)
def seq_cases():
    return [cut_case(16, 12), cut_case(8, 16)]


def seq_gens(kin):
    return [kin, 1, 2 * kin + 1, kin - 1, 3 * kin]


@functools.lru_cache(maxsize=None)
def two_per_cu_case(nw):
    """The first board (narrowest, then shortest) that the planner gives two tiles per CU: H <= 4096, W a multiple of
    64 up to 8192, the four depths, ``tiles`` in {1, 2, 3, 4, 8}.  None when there is none."""
    for W in range(64, 8193, 64):
        for H in range(MIN_H, 4097):
            for kin in DEPTHS:
                for tiles in (1, 2, 3, 4, 8):
                    p = plan(H, W, kin, tiles, nw)
                    if p and p.per_cu == 2:
                        return Case(H, W, kin, tiles, nw, p.B)
    return None


# ----- numpy references -----

_boards = {}


def board_after(H, W, gens):
    """wide_cases.start_board(H, W) after ``gens`` generations of B3/S23 on the torus (numpy_step), stepped on from
    the latest board already known."""
    known = _boards.setdefault((H, W), {0: wc.start_board(H, W)})
    if gens not in known:
        g0 = max(g for g in known if g <= gens)
        b = numpy_step(known[g0], gens - g0)
        b.setflags(write=False)
        known[gens] = b
    return known[gens]
