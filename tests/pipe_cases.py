"""Shared by test_pipe_plans.py (CPU) and test_gpu_pipe_geometries.py (MI355X): step_pipe<NW, L, WRAPY>
(csrc/src/hip/pipe_kernel.hip) in its 24 geometries -- NW in {5, 7, 9, 11, 13, 16} waves per workgroup (one loader and
NW - 1 compute stages) x L in {1, 2, 3, 4} generations per stage, K = (NW - 1) L generations per pass -- with and
without STEP_WRAP_Y.

Here, with no GPU needed:

  * the kernel's constants, written once (test_pipe_plans.py reads them back from the source text);
  * a pure-Python mirror of the control flow of ``stage<L, RIN, Out>``: which branches a stage takes that streams n
    input rows (no arithmetic is mirrored), labelled with the stage's role, because the three roles are three
    instantiations: ``first`` reads the loader's ring and writes a ring, ``middle`` reads and writes compute rings,
    ``last`` stores to HBM;
  * a mirror of the loader: the source rows it issues, how often the stream crosses row h with STEP_WRAP_Y, whether it
    reuses ring slots;
  * the case lists, built from the mirrors by a greedy cover (as tile_cases.py does for the tile kernels): per geometry
    a dozen ``(H, rows_per_wave)`` boards of width wide_cases.TAIL_W whose bands between them take every reachable
    branch of every role, none of which can be dropped; the small boards (H == K, H == K + 1); the strips of the
    thread-rank tests;
  * the numpy references: wide_cases.history, B3/S23 on the torus from seed 17, one history of GENS_TOTAL generations
    per board shared by every geometry.

Band heights are controlled through ``rows_per_wave``: a board of H rows is cut into ceil(H / rows_per_wave) bands of
H // n or H // n + 1 rows (wide_cases.equal_rows_bands), so a band shorter than K rows is a band of a board that still
has K rows, which the engine needs (the halo depth is clamped to the rows).  ``rows_per_wave`` is always given: the
pipe plan's own default depends on the CU count."""
import collections
import functools

import wide_cases as wc
from wide_cases import CONWAY

# ----- constants of the kernel (pipe_kernel.hip) -----
SYNC = 3         # kPipeSync: rows between counter updates
QUEUE = 3        # kPipeU: rows of a stage's register queue
RING = 18        # kPipeRing: rows of a ring between compute stages, and of one unrolled loop turn
RING0 = 18       # kPipeRing0: rows of the loader's ring
LOAD_AHEAD = 12  # kPipeLoadAhead: rows the loader keeps in flight
WAVES = [5, 7, 9, 11, 13, 16]
LEVELS = [1, 2, 3, 4]
GEOMETRIES = [(nw, L) for nw in WAVES for L in LEVELS]
DEFAULT = (9, 3)
ROLES = ["first", "middle", "last"]
NROWS_MAX = 400  # band heights of the brute-force search for reachable features


def depth(nw, L):
    return (nw - 1) * L


def gid(g):
    return f"{g[0]}-{g[1]}"


def i0(L):
    """stage's fill rows: the first multiple of 3 at which the L-level window is full."""
    return ((2 * L + 2) // 3) * 3


def kernel_name(nw, L, wg=1):
    """stats()["kernel"] of a pinned run, and a pass of a ``cut<R>=`` entry of stats()["tuning"]."""
    return f"pipe@{depth(nw, L)}({nw - 1}x{L},{wg}/CU)"


def cut(R, nw, L, wg=1, rest=()):
    """The ``cut<R>=`` entry for supersteps of R generations: whole step_pipe passes, then step_temporal passes of
    the depths ``rest``."""
    K = depth(nw, L)
    assert R - sum(rest) == R // K * K and sum(rest) < K
    return f"cut{R}=" + "+".join([kernel_name(nw, L, wg)] * (R // K) + [f"temporal@{d}" for d in rest])


GENS_TOTAL = 2 * max(depth(*g) for g in GEOMETRIES) + 1  # the shared history: 2K + 1 generations for every K


def gens_of(K):
    return 2 * K + 1


def conway_after(H, W, gens, total=GENS_TOTAL):
    """The B3/S23 torus board after ``gens`` (odd) generations from wide_cases' start board."""
    return wc.history(H, W, CONWAY, "torus", total)[1][gens]


# ----- the mirror of stage<L, RIN, Out>(in, out, n) -----

def stage_features(L, n):
    """The branches a stage of L levels takes on n input rows, by name:

    short             n <= i0: the fill ends the stream (the return inside the fill)
    queue_partial     i0 < n < i0 + 3: the prefetch queue is zero-filled past row n
    steady0/1/2plus   turns of the steady loop (while i + 18 + 3 <= n)
    rem=r             r = n - i rows left at the first tail pass
    tail2             the second tail pass runs (i + 18 < n)
    refill_full / refill_partial1 / refill_partial2 / refill_none
                      a tail pass's refill at the end of a row triple: three rows left to read, one, two, or none
    """
    first = i0(L)
    if n <= first:
        return {"short"}
    out = set()
    if n < first + QUEUE:
        out.add("queue_partial")
    i, turns = first, 0
    while i + RING + QUEUE <= n:
        i += RING
        turns += 1
    out.add(("steady0", "steady1")[turns] if turns < 2 else "steady2plus")
    out.add(f"rem={n - i}")
    starts = [i]
    if i + RING < n:
        out.add("tail2")
        starts.append(i + RING)
    for s in starts:
        for r in range(RING):
            if s + r >= n:
                break
            if r % SYNC != SYNC - 1:
                continue
            nx = s + r - (SYNC - 1) + QUEUE
            if nx + SYNC <= n:
                out.add("refill_full")
            elif nx < n:
                out.add(f"refill_partial{n - nx}")
            else:
                out.add("refill_none")
    return out


def role_of(nw, st):
    return "first" if st == 0 else ("last" if st == nw - 2 else "middle")


def stage_rows(nw, L, nrows, st):
    """Input rows of compute stage st (wave st + 1) of a segment of nrows rows."""
    return nrows + 2 * depth(nw, L) - 2 * st * L


def band_features(nw, L, nrows):
    """``role:feature`` of every stage of a segment of nrows rows."""
    out = set()
    for st in range(nw - 1):
        role = role_of(nw, st)
        out |= {f"{role}:{f}" for f in stage_features(L, stage_rows(nw, L, nrows, st))}
    return out


# ----- the mirror of loader<WRAPY>(src, d, p, K, n, ...) -----

Load = collections.namedtuple("Load", "rows published crossings prewrap")


def loader(K, h, row0, nrows, wrapy):
    """The loader's stream for a segment of rows [row0, row0 + nrows) of a tile of h rows: the source rows it issues
    in order (with STEP_WRAP_Y rows of the tile, else rows relative to the tile, negative and >= h in the ghost rows),
    how many of them it publishes, how often the wrapped row counter passes h, and whether it started below row 0."""
    n = nrows + 2 * K
    lrow = row0 - K
    prewrap = wrapy and lrow < 0
    if prewrap:
        lrow += h
    rows, crossings = [], 0
    for _ in range(max(LOAD_AHEAD, n)):  # the first LOAD_AHEAD unconditionally, then one per published row
        rows.append(lrow)
        lrow += 1
        if wrapy and lrow == h:
            lrow = 0
            crossings += 1
    return Load(rows, n, crossings, prewrap)


def n0_class(n0):
    if n0 <= LOAD_AHEAD:
        return "loader:n0<=12"  # nothing issued in the loop
    return "loader:n0<=18" if n0 <= RING0 else "loader:n0>18"  # beyond 18: slots reused, the loader waits


def loader_features(K, h, row0, nrows, wrapy=True):
    out = {n0_class(nrows + 2 * K)}
    if wrapy:
        ld = loader(K, h, row0, nrows, True)
        out.add(f"loader:cross={min(ld.crossings, 2)}" + ("+" if ld.crossings >= 2 else ""))
        top, bottom = row0 == 0, row0 + nrows == h
        out.add("loader:band=" + ("single" if top and bottom else "top" if top else "bottom" if bottom else "middle"))
        if h == K:
            out.add("loader:h==K")
    return out


POSITIONS = {"loader:cross=0", "loader:cross=1", "loader:cross=2+", "loader:band=single", "loader:band=top",
             "loader:band=bottom", "loader:band=middle"}


# ----- what a geometry's cases must reach -----

@functools.lru_cache(maxsize=None)
def reachable(nw, L):
    """Every stage feature and loader row-count class some band of 1 .. NROWS_MAX rows has, and the loader's positions:
    a single band, the top, the bottom and a middle band of several, and a stream that passes row h never (a middle
    band of a board of more than 2K + 2 rows), once and twice."""
    out = set(POSITIONS)
    for nrows in range(1, NROWS_MAX + 1):
        out |= band_features(nw, L, nrows)
        out.add(n0_class(nrows + 2 * depth(nw, L)))
    return frozenset(out)


Case = collections.namedtuple("Case", "H rows")  # rows: rows_per_wave


def case_features(nw, L, c):
    out = set()
    for row0, nrows in wc.equal_rows_bands(c.H, c.rows):
        out |= band_features(nw, L, nrows) | loader_features(depth(nw, L), c.H, row0, nrows)
    return out - {"loader:h==K"}  # (the small boards' feature: small_cases below)


# The boards the loop-tail cases are chosen from: heights that every geometry can run (K <= 60), so that the 24
# geometries share their numpy histories.  Cut by rows_per_wave into 1 .. H bands, 60 .. 77 rows give every band
# height 1 .. 25, 30 .. 38 and 60 .. 77; 124 rows hold a band whose 2K + 3 streamed rows stay inside the board at
# K = 60 (no crossing of row h), which below 2K + 2 rows no band does.
POOL = list(range(60, 78)) + [124]


def universe():
    seen = set()
    for H in POOL:
        for rows in range(H, 0, -1):
            bands = tuple(wc.equal_rows_bands(H, rows))
            if bands not in seen:  # (rows_per_wave values that cut alike)
                seen.add(bands)
                yield Case(H, rows)


@functools.lru_cache(maxsize=None)
def loop_tail_cases(nw, L):
    """A few boards of ``universe()`` whose bands between them have every feature of ``reachable(nw, L)``: a greedy
    cover, the first board (the shortest, in the fewest bands) among those that add the most, then every board dropped
    that the others make redundant, so that none can be removed without losing a feature."""
    cand = dict((c, case_features(nw, L, c)) for c in universe())
    want = set(reachable(nw, L))
    left, chosen = set(want), []
    while left:
        c = max(cand, key=lambda c: len(cand[c] & left))  # (max keeps the first of equals)
        if not cand[c] & left:
            break
        chosen.append(c)
        left -= cand[c]
    for c in list(chosen):
        rest = [x for x in chosen if x != c]
        if want - left <= set().union(*(cand[x] for x in rest)):
            chosen = rest
    return tuple(chosen)


def covered(nw, L, cases):
    out = set()
    for c in cases:
        out |= case_features(nw, L, c)
    return out


# ----- the small boards: H == K and H == K + 1 -----

SMALL_WIDTHS = [64, 65, 128]  # one word that is its own x neighbour; a one-cell tail word; two words

Small = collections.namedtuple("Small", "H W rows")


def small_cases(nw, L):
    """H == K: the loader's first row is the segment's own first row and a single band's stream passes row h three
    times; H == K + 1.  Each as one band and as bands of one row."""
    K = depth(nw, L)
    return [Small(H, W, rows) for H in (K, K + 1) for W in SMALL_WIDTHS for rows in (H, 1)]


# ----- wide shapes -----

def wide_cases(nw, L):
    """The shapes of wide_cases.SHAPES with at least K rows, cut into two bands."""
    return [s for s in wc.SHAPES if depth(nw, L) <= s.H]


def wide_rows(s):
    return s.H // 2


TALL_GEOMETRIES = [g for g in GEOMETRIES if gens_of(depth(*g)) <= wc.TALL_GENS]  # (5,1), (7,1), (5,2), (9,1)

# ----- thread ranks: no STEP_WRAP_Y -----

Strip = collections.namedtuple("Strip", "h rows")  # a rank's strip of h rows cut at ``rows`` rows per band

GHOST_ORDINARY, GHOST_TALL = 45, 83  # bands of 23 / 22 rows; of 42 / 41 rows (two steady turns of the last stage)


def ghost_strips(nw, L):
    """Only the loader differs from STEP_WRAP_Y (the stages are covered by loop_tail_cases), so three strips: one whose
    loader never reuses a ring slot (n0 <= 18: K <= 8 only; two bands, at K = 8 four bands of two rows, since a strip
    has at least K rows), one ordinary, one of bands of more than 40 rows.  Every strip has at least K rows."""
    K = depth(nw, L)
    out = []
    if 2 * K + 1 <= RING0:
        nr = RING0 - 2 * K
        out.append(Strip(max(2 * nr, K), nr))
    for h in (GHOST_ORDINARY, GHOST_TALL):
        h = max(h, K + 1)
        out.append(Strip(h, (h + 1) // 2))
    return out


MULTI = wc.Shape(96, 4096, 1, 2, 64)   # P = 2: strips of 48 x 4096
MULTI_ROWS = 24
MULTI_GEOMETRIES = [(7, 1), (11, 2), (5, 3), (5, 4), DEFAULT]  # one per L and the default: 2K <= 48 rows
GRID = wc.Shape(96, 8192, 2, 4, 64)    # 2 x 2: tiles of 48 x 4096
GRID_GEOMETRIES = [(7, 1), (5, 2), (5, 3), (5, 4)]  # one per L, 2K <= 63: the ghost words stay exact
