"""Shared by test_tile_plans.py (CPU) and test_gpu_tile.py (MI355X): the LDS tile kernels step_tile and
step_tile_fold (csrc/src/hip/tile_device.hpp) in their 72 variants: NW in {4, 8, 16} waves per workgroup x LV in
{1, 2, 4} generations per LDS pass x double-buffered / in place x plain / folded x WRAPY on / off.

Here, with no GPU needed:

  * a pure-Python mirror of the kernels' band arithmetic: the LDS passes ``(g, lv)`` of a tile at depth K
    (tile_item / fold_item) and, per pass, every wave's band ``(r0, r1, n)`` (tile_pass / fold_pass), for folded tiles
    with T, Th, the mirrored rows and T's parity;
  * mirrors of tile_max_rows and tile_lds_rows for the four buffer layouts;
  * the case lists, built from those mirrors by a greedy cover of the features each variant must meet (every tail of
    tile_band's loops, idle waves, short last bands, bands thinner than LV, the remainder passes, T's parity, the
    mirror rows written by several waves, the shortest and tallest short folded tiles), over the smallest boards;
  * the numpy references (wide_cases.history: B3/S23 on the torus, computed once per board);
  * a failure report in the plan's terms: wrong cells, the first one's row, word and tile, whether its row lies in the
    first or last K rows of its tile, and for folded tiles its distance from the middle row.

The tile height is controlled two ways: a board of H rows with ``rows_per_wave >= H`` is one tile of H rows (WRAPY);
a board cut by an explicit ``rows_per_wave`` has the balanced band heights of pack_waves (wide_cases.equal_rows_bands).
Folded tiles shorter than kFoldMinRows = 28 rows exist only as bands of a taller region: H = 29 .. 55 rows at
``rows_per_wave = 28`` are two tiles of 14 .. 28 rows."""
import collections
import functools
import itertools

import numpy as np

import wide_cases as wc
from wide_cases import CONWAY

# ----- constants of the kernels (tile_device.hpp, step_kernels.hip, hip_kernels.hpp) -----
LDS_ROWS = 320        # 160 KiB of LDS in rows of 512 B
FOLD_MIRROR = 4       # kFoldMirror
FOLD_MIN_ROWS = 28    # kFoldMinRows
FOLD_SEG = 30         # output words of a full-width folded segment (32 lanes with the two halo lanes)
KERNEL_MAX_DEPTH = 64  # launch_step_tile
ENGINE_MAX_DEPTH = 32  # HipEngine: kernel "tile" runs passes of at most 32 generations
WAVES = [4, 8, 16]
LEVELS = [1, 2, 4]
SEED = wc.SEED

Variant = collections.namedtuple("Variant", "nw lv inplace fold")
VARIANTS = [Variant(nw, lv, ip, fold) for fold in (False, True) for ip in (False, True) for lv in LEVELS for nw in WAVES]


def layout(v):
    """The buffer layout's name in the ``tile_plan=`` entry of stats()["tuning"]."""
    return ("fold-inplace" if v.inplace else "fold") if v.fold else ("inplace" if v.inplace else "double")


def vid(v):
    return f"{layout(v)}-nw{v.nw}-lv{v.lv}"


def entry(name, v, rows, tiles):
    """The ``tile_plan=`` (one tile, full schedule), ``tile_plan1=`` / ``tile_plan2=`` (split: interior, bands) entry."""
    return f"{name}={layout(v)},{rows}rows,{tiles}tiles,lv{v.lv}"


# ----- the band arithmetic -----

def side_rows(lv):
    return 2 * lv + 4


def passes(K, LV):
    """The LDS passes ``(g, lv)`` of K generations at up to LV levels per pass (tile_item / fold_item)."""
    out, g = [], 0
    while g < K:
        left = K - g
        lv = 4 if LV >= 4 and left >= 4 else (2 if LV >= 2 and left >= 2 else 1)
        out.append((g, lv))
        g += lv
    return out


Band = collections.namedtuple("Band", "wv r0 r1 n")  # output rows [r0, r1), n streamed rows (0: an idle wave)
Pass = collections.namedtuple("Pass", "g lv last cnt b bands")


def _split(lo_r, cnt, NW, lv):
    b = -(-cnt // NW)
    bands = []
    for wv in range(NW):
        r0 = lo_r + wv * b
        r1 = min(r0 + b, lo_r + cnt)
        bands.append(Band(wv, r0, r1, r1 - r0 + 2 * lv if r1 > r0 else 0))
    return b, bands


def plain_passes(nrows, K, NW, LV):
    """tile_pass: the pass at generation g computes tile rows [g + lv, n_in - g - lv) of n_in = nrows + 2K."""
    n_in = nrows + 2 * K
    out = []
    for g, lv in passes(K, LV):
        cnt = n_in - 2 * g - 2 * lv
        b, bands = _split(g + lv, cnt, NW, lv)
        out.append(Pass(g, lv, g + lv >= K, cnt, b, bands))
    return out


Fold = collections.namedtuple("Fold", "T Th m_lo m_hi odd")


def fold_geometry(nrows, K):
    """T staged rows, Th virtual rows per half, virtual rows m_lo .. m_hi mirrored into the other half's lanes
    (FoldSink); T odd: both halves compute and store the middle row."""
    T = nrows + 2 * K
    Th = (T + 1) // 2
    return Fold(T, Th, T - Th - FOLD_MIRROR, T - 1 - Th, T % 2 == 1)


def fold_passes(nrows, K, NW, LV):
    """fold_pass: the pass at generation g computes virtual rows [g + lv, Th) of both halves."""
    f = fold_geometry(nrows, K)
    out = []
    for g, lv in passes(K, LV):
        cnt = f.Th - g - lv
        b, bands = _split(g + lv, cnt, NW, lv)
        out.append(Pass(g, lv, g + lv >= K, cnt, b, bands))
    return out


def tile_passes(v, nrows, K):
    return (fold_passes if v.fold else plain_passes)(nrows, K, v.nw, v.lv)


def mirror_writers(f, p):
    """The waves of a pass that write one of the mirrored rows (the last pass stores to HBM: none)."""
    if p.last:
        return []
    return [b.wv for b in p.bands if b.n and b.r0 <= f.m_hi and b.r1 > f.m_lo]


# ----- LDS capacity -----

def fold_buffer_rows(T):
    return (T + 1) // 2 + FOLD_MIRROR + 4


def lds_rows(v, rows, K):
    """tile_lds_rows: the LDS rows a tile of ``rows`` output rows takes at depth K."""
    if v.fold:
        fb = fold_buffer_rows(rows + 2 * K)
        return fb + v.nw * side_rows(v.lv) if v.inplace else 2 * fb
    return rows + 2 * K + v.nw * side_rows(v.lv) if v.inplace else 2 * (rows + 2 * K) + 4


def max_rows(v, K):
    """tile_max_rows: the most output rows of a tile at depth K."""
    if v.fold:
        if v.inplace:
            return 2 * (LDS_ROWS - v.nw * side_rows(v.lv) - FOLD_MIRROR - 4) - 1 - 2 * K
        return 2 * (LDS_ROWS // 2 - FOLD_MIRROR - 4) - 1 - 2 * K
    if v.inplace:
        return LDS_ROWS - v.nw * side_rows(v.lv) - 2 * K
    return (LDS_ROWS - 4) // 2 - 2 * K


# ----- boards, tiles and what the planner does with them -----

Case = collections.namedtuple("Case", "H W K rows")  # rows: rows_per_wave


def tiles_of(H, rows):
    """``[(row0, nrows)]``: the tiles of a region of H rows cut at ``rows`` rows per tile (pack_waves)."""
    return wc.equal_rows_bands(H, rows)


def folds(region_rows, rows):
    """HipEngine::plan with GOL_TILE_FOLD=1: a plan folds when its tallest region has kFoldMinRows rows and its
    thinnest kFoldMinRows / 2; ``rows_per_wave`` must then be at least kFoldMinRows (the engine refuses less)."""
    return max(region_rows) >= FOLD_MIN_ROWS and min(region_rows) >= FOLD_MIN_ROWS // 2 and rows >= FOLD_MIN_ROWS


def plan_tiles(gol, regions, W, H, rows, K, fold, x_wrap=None):
    """The tiles ``build_plan`` makes of ``regions`` (``[(r0, r1, c0, c1)]``): ``(waves, stats)`` as wide_cases.build."""
    nw = wc.nwords(W)
    x_wrap = wc.xwrap(W, "torus") if x_wrap is None else x_wrap
    lanes, stats = gol.native.build_plan([tuple(int(x) for x in r) for r in regions], nw, H, rows, K, x_wrap, fold)
    lanes = np.asarray(lanes).reshape(-1, wc.LANES, 4)
    waves = []
    for i, w in enumerate(lanes):
        assert len(set(w[:, 3].tolist())) == 1, f"tile {i}: nrows differs between lanes"
        if w[0, 3] > 0:
            waves.append(wc.Wave(i, w[:, 0].copy(), w[:, 1].copy(), (w[:, 2] & wc.LANE_STORE) != 0, int(w[0, 3])))
    return waves, stats


# ----- features a variant's cases must reach -----

def fill_rows(lv):
    """tile_band's i0: the fill loop streams rows 0 .. i0 - 1 under guards, three per turn."""
    return (2 * lv + 2) // 3 * 3


def steady_from(lv):
    """The least n at which tile_band's steady loop runs a turn: the two-triple loop (6 rows) at 4 levels, else the
    single-triple loop (3 rows).  Below it a band is streamed by the fill loop and the tail rows alone."""
    return fill_rows(lv) + (6 if lv == 4 else 3)


def loop_mod(lv):
    return 6 if lv == 4 else 3


def stream_feature(lv, n):
    """What a band of n streamed rows exercises in the lv-level band stream: below the steady loop n itself (every such
    n differs in which guards of the fill loop hold); from it on, n modulo the steady loop's stride, which picks what
    follows the loop: a leftover triple at 4 levels, 0 - 2 tail rows."""
    return f"fill n={n}" if n < steady_from(lv) else f"steady n%{loop_mod(lv)}={n % loop_mod(lv)}"


def max_staged_rows(v):
    """The most rows a tile may stage, nrows + 2K, whatever the depth (max_rows(v, K) + 2K)."""
    return max_rows(v, 0)


def max_band_rows(v):
    """The tallest band of an LV-level pass the LDS capacity allows: the first pass of the tallest tile."""
    T = max_staged_rows(v)
    cnt = ((T + 1) // 2 - v.lv) if v.fold else T - 2 * v.lv
    return -(-cnt // v.nw)


def required(v):
    """What the cases of variant ``v`` must contain between them (test_tile_plans.py asserts it)."""
    req = [f"fill n={n}" for n in range(2 * v.lv + 1, steady_from(v.lv))]
    req += [f"steady n%{loop_mod(v.lv)}={r}" for r in range(loop_mod(v.lv))]
    req += ["idle-wave", "short-last-band", "band<LV", "passes-odd", "passes-even"]
    if v.lv > 1:
        req += [f"K%{v.lv}={r}" for r in range(v.lv)]
    if v.fold:
        req += ["T-odd", "T-even", "mirror-2-waves", "middle-band-alone"]
        req += [f"rows={r}" for r in (FOLD_MIN_ROWS // 2, FOLD_MIN_ROWS // 2 + 1, FOLD_MIN_ROWS - 1, FOLD_MIN_ROWS)]
    return req


def features(v, nrows, K):
    """The features of one tile of ``nrows`` rows at depth K under variant ``v``.  The band-stream features count the
    passes that run the variant's own LV-level stream (remainder passes run the 2- and 1-level streams)."""
    ps = tile_passes(v, nrows, K)
    out = {"passes-odd" if len(ps) % 2 else "passes-even"}
    if v.lv > 1:
        out.add(f"K%{v.lv}={K % v.lv}")
    for p in ps:
        live = [b for b in p.bands if b.n]
        if len(live) < v.nw:
            out.add("idle-wave")
        if live[-1].r1 - live[-1].r0 < p.b and len(live) > 1:
            out.add("short-last-band")
        if len(live) == 1:
            out.add("middle-band-alone")
        if p.lv != v.lv:
            continue
        for b in live:
            out.add(stream_feature(v.lv, b.n))
            if b.r1 - b.r0 < v.lv:
                out.add("band<LV")
    if v.fold:
        f = fold_geometry(nrows, K)
        out.add("T-odd" if f.odd else "T-even")
        out.add(f"rows={nrows}")
        if any(len(mirror_writers(f, p)) >= 2 for p in ps):
            out.add("mirror-2-waves")
    return out


def case_features(v, c):
    out = set()
    for _, n in tiles_of(c.H, c.rows):
        out |= features(v, n, c.K)
    return out


def unreachable(v):
    """Required features no tile of variant ``v`` can have, each with its reason from the mirror."""
    out = {}
    if v.lv == 1:
        out["band<LV"] = "every band of a pass has at least one row, and LV = 1"
    # the steady loop's residues: a band has at most max_band_rows(v) rows, so n takes 2 LV + 1 .. that + 2 LV only
    top = max_band_rows(v) + 2 * v.lv
    reach = {stream_feature(v.lv, n) for n in range(2 * v.lv + 1, top + 1)}
    for f in required(v):
        if (f.startswith("steady") or f.startswith("fill")) and f not in reach:
            out[f] = (f"the LDS holds at most {max_staged_rows(v)} staged rows, so a band of {v.nw} waves has at most "
                      f"{max_band_rows(v)} rows and streams n <= {top} rows: {sorted(reach)} only")
    if v.fold:
        # a pass of a folded tile has cnt = Th - g - lv >= Th - K = ceil(nrows / 2) >= kFoldMinRows / 4 rows, cut into
        # bands of ceil(cnt / NW) rows: one band only if cnt <= ceil(cnt / NW), that is cnt = 1
        least = -(-(FOLD_MIN_ROWS // 2) // 2)
        out["middle-band-alone"] = (f"a folded tile has at least {FOLD_MIN_ROWS // 2} rows, so every pass computes at "
                                    f"least {least} virtual rows, and {least} rows over {v.nw} waves are "
                                    f"{len([b for b in _split(0, least, v.nw, 1)[1] if b.n])} bands")
    return out


COLS = 192          # narrow packed segments: 3 words
SWEEP_DEPTHS = list(range(1, 14))
FOLD_ROWS = FOLD_MIN_ROWS
FOLD_HEIGHTS = list(range(FOLD_MIN_ROWS, 2 * FOLD_MIN_ROWS))  # 28: one tile; 29 .. 55: two tiles of 14 .. 28 rows


def universe(v, W=COLS):
    """The boards the cases are chosen from, by staged rows H + 2K, smallest first, up to the LDS capacity.  Plain: one
    tile of H >= K rows (the halo depth is at most H).  Folded: H = 28 .. 55 rows cut at 28 (one tile of 28 rows, two
    of 14 .. 28), then one tile of H rows."""
    for T in range(3, max_staged_rows(v) + 1):
        for K in SWEEP_DEPTHS:
            H = T - 2 * K
            if H < K:
                continue
            if not v.fold:
                yield Case(H, W, K, H)
            elif H in FOLD_HEIGHTS:
                yield Case(H, W, K, FOLD_ROWS)
            elif H > FOLD_HEIGHTS[-1]:
                yield Case(H, W, K, H)


@functools.lru_cache(maxsize=None)
def sweep_cases(v, W=COLS):
    """The fewest boards of ``universe(v)`` that between them have every reachable feature of ``required(v)``: a greedy
    cover, the smallest board first among those that add the most.  (The universe is read smallest first, only as far
    as it takes to meet every feature.)"""
    want = {f for f in required(v) if f not in unreachable(v)}
    cand, seen = [], set()
    for c in universe(v, W):
        if want <= seen:
            break
        cand.append((c, case_features(v, c)))
        seen |= cand[-1][1]
    left, chosen = set(want), []
    while left:
        c, fs = max(cand, key=lambda cf: len(cf[1] & left))  # (max keeps the first of equals: the smallest)
        if not fs & left:
            break
        chosen.append(c)
        left -= fs
    return tuple(chosen)


def covered(v, cases):
    out = set()
    for c in cases:
        out |= case_features(v, c)
    return out


# ----- further case lists of test_gpu_tile.py -----

DEPTH_SWEEP = [1, 2, 3, 4, 5, 7, 8, 13, 24, 32, 48, 64]
DEFAULT = Variant(8, 4, False, False)       # HipEngine::tile_bits: 8 waves, double-buffered: 4 levels
DEFAULT_FOLD = Variant(8, 4, False, True)
CAPACITY_DEPTHS = [8, 32]
CAPACITY_WAVES = [4, 16]
FULL_FOLD = [1920, 2048]                    # 30 words: one full 32-lane folded segment; 32 words: 30 + 2
WIDE = [wc.S3968, wc.S3950, wc.S4096, wc.S8000]
WIDE_DEPTHS = [5, 8]
SPLIT_BOARDS = [(1024, 192), (96, 4096)]
SPLIT_DEPTHS = [5, 16]
SPLIT_ROWS = 32                             # rows_per_wave of the split tests: the bands are one tile each
RANKS_BOARD = (96, 4096)
RANKS_DEPTHS = [4, 8]
CROSS_BOARDS = [(wc.S8000.H, wc.S8000.W), (64, 1920)]
CROSS_DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8]


def engine_cut(K):
    """``(S, depths)``: the supersteps and their passes when kernel_depth = halo_depth = K on one rank.  Up to 32 one
    pass of K; beyond, the engine caps the pass at 32 and a rank without neighbours cuts its supersteps at the largest
    multiple of the pass depth within K (HipEngine::superstep_depth): 48 runs supersteps of one pass of 32, 64 of two."""
    if K <= ENGINE_MAX_DEPTH:
        return K, [K]
    S = K // ENGINE_MAX_DEPTH * ENGINE_MAX_DEPTH
    return S, [ENGINE_MAX_DEPTH] * (S // ENGINE_MAX_DEPTH)


def tile_cut(R, depths):
    return f"cut{R}=" + "+".join(f"tile@{d}" for d in depths)


def split_regions(H, nw, K):
    """HipEngine::regions of a rank that is its own neighbour: the interior (kind 1) and the two bands (kind 2)."""
    return [(K, H - K, 0, nw)], [(0, K, 0, nw), (H - K, H, 0, nw)]


# ----- references -----

def gens_of(K):
    return 2 * K + 1


@functools.lru_cache(maxsize=None)
def reference(H, W, gens):
    """The B3/S23 torus board after ``gens`` generations from wide_cases' start board (numpy, computed once)."""
    return wc.history(H, W, CONWAY, "torus", gens)[1][gens]


def phase_board(W=COLS):
    """A board that holds every one of the 512 3 x 3 neighbourhoods centred on a row of each phase mod 3, in an even
    and in an odd column: six stacks of the 512 patterns, 4 rows and 4 columns apart, stack s starting on a row that
    is s % 3 mod 3 and shifted right by s // 3 columns.  test_gpu_tile.py asserts the property with
    ``neighbourhoods_seen``.  The height is a multiple of 3, so the phases hold across the torus seam."""
    per_row = W // 4
    block_rows = 4 * (-(-512 // per_row))
    H = 6 * (block_rows + 2)
    H += -H % 3
    b = np.zeros((H, W), np.uint8)
    for s in range(6):
        dr, dc = s % 3, s // 3
        base = s * (block_rows + 2)
        base += (dr - base) % 3  # the centre rows of stack s are base + 1 + 4i: phase (dr + 1) % 3
        for p in range(512):
            r, c = base + 4 * (p // per_row), 4 * (p % per_row) + dc
            for i in range(9):
                b[(r + i // 3) % H, (c + i % 3) % W] = (p >> i) & 1
    b.setflags(write=False)
    return b


def neighbourhoods_seen(b):
    """``seen[phase][parity]``: the set of 3 x 3 neighbourhoods (9-bit codes, row-major from the top left) centred on a
    row of that phase mod 3 and a column of that parity."""
    H, W = b.shape
    code = np.zeros((H, W), np.int32)
    for i in range(9):
        code |= np.roll(np.roll(b, 1 - i // 3, 0), 1 - i % 3, 1).astype(np.int32) << i
    return [[set(code[ph::3, par::2].ravel().tolist()) for par in range(2)] for ph in range(3)]


# ----- where a wrong board is wrong -----

def tile_report(got, ref, K, tiles, fold=False, seg=wc.SEG):
    """Where ``got`` differs from ``ref`` in the plan's terms (``tiles``: ``[(row0, nrows)]``): the number of wrong
    cells, the first one's row, word and tile, whether its row lies in the first or last K rows of its tile and, for a
    folded tile, how far it is from the middle row of the T = nrows + 2K staged rows."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return f"shapes differ: {got.shape} against {ref.shape}"
    bad = got != ref
    if not bad.any():
        return ""
    rows, cols = np.nonzero(bad)
    r, c = int(rows[0]), int(cols[0])
    lines = [f"{int(bad.sum())} of {bad.size} cells differ in {len(set(rows.tolist()))} rows",
             f"first wrong cell: row {r}, column {c} = word {c // 64} (word {c // 64 % seg} of segment {c // 64 // seg})"]
    for i, (r0, n) in enumerate(tiles):
        if r0 <= r < r0 + n:
            where = [name for name, hit in (("first", r - r0 < K), ("last", r0 + n - r <= K)) if hit]
            lines.append(f"tile {i} of {len(tiles)}: rows {r0} .. {r0 + n - 1}; tile row {r - r0}, " +
                         (f"in its {' and '.join(where)} {K} rows" if where else "inside"))
            if fold:
                f = fold_geometry(n, K)
                t = r - r0 + K
                lines.append(f"folded: T = {f.T} ({'odd' if f.odd else 'even'}), staged row {t} of half "
                             f"{0 if t < f.Th else 1}, {abs(2 * t - (f.T - 1)) / 2:g} rows from the middle")
            break
    else:
        lines.append("outside every tile")
    edge = sum(1 for x in set(rows.tolist()) for r0, n in tiles if r0 <= x < r0 + n and (x - r0 < K or r0 + n - x <= K))
    lines.append(f"{edge} of the wrong rows lie in the first / last {K} rows of a tile")
    return "\n".join(lines)


def check_board(got, ref, K, tiles, fold=False, seg=wc.SEG):
    assert np.array_equal(got, ref), tile_report(got, ref, K, tiles, fold, seg)


# every __global__ instantiation: kernel, NW, WRAPY, LV, in place
INSTANTIATIONS = [(("step_tile_fold" if fold else "step_tile"), nw, wrapy, lv, ip)
                  for fold, nw, wrapy, lv, ip in itertools.product((False, True), WAVES, (True, False), LEVELS, (False, True))]
