"""The case lists of tile_cases.py really contain what test_gpu_tile.py relies on: per variant of step_tile /
step_tile_fold (NW x LV x in place x fold) every tail of tile_band's loops, an idle wave, a short last band, a band
thinner than LV, every remainder pass and both parities of the buffer swaps; for folded tiles both parities of T,
mirror rows written by two waves and tiles of 14, 15, 27 and 28 rows.  All of it is recomputed here from the mirror of
the kernels' band arithmetic, so a change of the planner or of a constant cannot quietly turn the GPU tests into easy
cases.  A feature a variant cannot reach at all is named with its reason and shown unreachable over every board the
cases are chosen from.  The plans come from ``build_plan`` with the engine's arguments.  No GPU is needed."""
import numpy as np
import pytest

import tile_cases as tc
import wide_cases as wc
from tile_cases import VARIANTS, vid


# ----- the mirror itself -----

def test_passes():
    assert tc.passes(13, 4) == [(0, 4), (4, 4), (8, 4), (12, 1)]
    assert tc.passes(7, 4) == [(0, 4), (4, 2), (6, 1)]
    assert tc.passes(5, 2) == [(0, 2), (2, 2), (4, 1)]
    assert tc.passes(3, 1) == [(0, 1), (1, 1), (2, 1)]
    for K in range(1, tc.KERNEL_MAX_DEPTH + 1):
        for LV in tc.LEVELS:
            ps = tc.passes(K, LV)
            assert sum(lv for _, lv in ps) == K and all(lv <= LV for _, lv in ps)
            assert [g for g, _ in ps] == [sum(lv for _, lv in ps[:i]) for i in range(len(ps))]


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_bands_tile_the_pass(v):
    """Every pass's live bands are disjoint, in wave order and cover exactly its output rows; every streamed row is a
    row of the tile's LDS buffer (plain) or a virtual row up to the last mirror (folded)."""
    for nrows in (1, 2, 5, 14, 15, 27, 28, 29, 64, 100):
        if v.fold and nrows < tc.FOLD_MIN_ROWS // 2:
            continue
        for K in (1, 2, 3, 4, 5, 7, 8, 13, 24, 32, 64):
            f = tc.fold_geometry(nrows, K)
            for p in tc.tile_passes(v, nrows, K):
                live = [b for b in p.bands if b.n]
                lo, hi = (p.g + p.lv, f.Th) if v.fold else (p.g + p.lv, nrows + 2 * K - p.g - p.lv)
                assert p.cnt == hi - lo >= 1 and live[0].r0 == lo and live[-1].r1 == hi
                assert all(a.r1 == b.r0 for a, b in zip(live, live[1:]))
                assert all(b.n == b.r1 - b.r0 + 2 * p.lv and b.r0 - p.lv >= p.g for b in live)
                assert [b.wv for b in live] == list(range(len(live)))
                if v.fold:  # reads reach lv rows past Th: mirrors, staged and rewritten by every pass but the last
                    assert hi + p.lv <= f.Th + tc.FOLD_MIRROR and f.m_hi - f.m_lo + 1 == tc.FOLD_MIRROR
                    assert f.T - 1 - f.m_lo == f.Th + tc.FOLD_MIRROR - 1 and f.T - 1 - f.m_hi == f.Th
                    assert f.m_lo >= p.g + p.lv or p.last or f.m_lo >= K  # the mirrored rows are outputs of the pass
                    assert f.Th + tc.FOLD_MIRROR + 4 <= f.T or K + nrows // 2 < 8  # staged rows are rows of the tile


def test_capacity_mirrors():
    """max_rows is the most rows whose LDS rows fit the 320 (a folded tile's T is kept odd: one more row, T even, takes
    the same buffers; two more do not fit)."""
    for v in VARIANTS:
        for K in range(1, tc.KERNEL_MAX_DEPTH + 1):
            cap = tc.max_rows(v, K)
            assert tc.lds_rows(v, cap, K) <= tc.LDS_ROWS < tc.lds_rows(v, cap + (2 if v.fold else 1), K), (v, K)
            if v.fold:
                assert (cap + 2 * K) % 2 == 1 and tc.lds_rows(v, cap + 1, K) == tc.lds_rows(v, cap, K)
    # the layouts at the benchmarked depth: 8 waves, K = 24
    assert [tc.max_rows(tc.Variant(8, lv, ip, fold), 24) for fold, ip, lv in
            [(False, False, 4), (False, True, 2), (True, False, 4), (True, True, 4)]] == [110, 208, 255, 383]
    # the deepest pass the kernel accepts leaves in-place tiles of 16 waves at 4 levels no row
    assert tc.max_rows(tc.Variant(16, 4, True, False), tc.KERNEL_MAX_DEPTH) == 0


def test_engine_depths():
    assert tc.engine_cut(13) == (13, [13]) and tc.engine_cut(32) == (32, [32])
    assert tc.engine_cut(48) == (32, [32]) and tc.engine_cut(64) == (64, [32, 32])
    assert tc.tile_cut(*tc.engine_cut(64)) == "cut64=tile@32+tile@32"


def test_instantiations():
    assert len(tc.INSTANTIATIONS) == len(set(tc.INSTANTIATIONS)) == 72 and len(VARIANTS) == len(set(VARIANTS)) == 36


# ----- the sweep's cases reach every feature -----

@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_sweep_cases_cover(v):
    """Recomputed from the bands, not from tile_cases.features."""
    cases = tc.sweep_cases(v)
    assert 1 <= len(cases) <= 6, cases
    mod = 6 if v.lv == 4 else 3
    ns, ks, swaps, heights, parities = set(), set(), set(), set(), set()
    idle = short = thin = two_writers = alone = False
    for c in cases:
        assert c.W == tc.COLS and c.K <= c.H and c.K <= tc.ENGINE_MAX_DEPTH
        tiles = tc.tiles_of(c.H, c.rows)
        assert sum(n for _, n in tiles) == c.H
        if v.fold:
            assert tc.folds([c.H], c.rows) and c.rows <= tc.max_rows(v, c.K), c
            assert all(n >= tc.FOLD_MIN_ROWS // 2 for _, n in tiles)
        else:
            assert len(tiles) == 1 and c.H <= tc.max_rows(v, c.K), c
        ks.add(c.K % v.lv)
        for _, nrows in tiles:
            heights.add(nrows)
            f = tc.fold_geometry(nrows, c.K)
            parities.add(f.odd)
            ps = tc.tile_passes(v, nrows, c.K)
            swaps.add(len(ps) % 2)
            for p in ps:
                live = [b for b in p.bands if b.n]
                idle |= len(live) < v.nw
                short |= len(live) > 1 and live[-1].r1 - live[-1].r0 < live[0].r1 - live[0].r0
                alone |= len(live) == 1
                two_writers |= v.fold and len(tc.mirror_writers(f, p)) >= 2
                if p.lv == v.lv:
                    ns |= {b.n for b in live}
                    thin |= any(b.r1 - b.r0 < v.lv for b in live)
    # tile_band: the fill loop ends at i0 = 3, 6, 9 rows; the steady loop's first turn takes 3, 3, 6 more
    first_steady = {1: 3 + 3, 2: 6 + 3, 4: 9 + 6}[v.lv]
    assert first_steady == tc.steady_from(v.lv)
    assert {n for n in ns if n < first_steady} == set(range(2 * v.lv + 1, first_steady)), sorted(ns)
    assert v.lv != 2 or 5 in ns  # a one-row band at 2 levels: the fill loop's guards end the stream
    # every residue of n from the steady loop on, as far as the tallest band the LDS allows reaches them
    tallest = tc.tile_passes(v, tc.max_rows(v, v.lv), v.lv)[0]
    assert tallest.lv == v.lv and tallest.b == tc.max_band_rows(v)
    assert tc.lds_rows(v, tc.max_rows(v, v.lv), v.lv) <= tc.LDS_ROWS
    can = {n % mod for n in range(first_steady, tallest.b + 2 * v.lv + 1)}
    assert {n % mod for n in ns if n >= first_steady} == can, sorted(ns)
    assert (can == set(range(mod))) == (not (v.nw == 16 and v.lv == 4)), (can, tallest)
    assert idle and short
    assert ks == set(range(v.lv)) and swaps == {0, 1}
    cannot = tc.unreachable(v)
    assert set(cannot) <= set(tc.required(v))
    assert thin == ("band<LV" not in cannot)
    if v.fold:
        assert parities == {True, False} and two_writers
        assert {14, 15, 27, 28} <= heights, sorted(heights)
        assert not alone and "middle-band-alone" in cannot
    assert set(tc.required(v)) - set(cannot) <= tc.covered(v, cases)


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_unreachable_features(v):
    """What a variant cannot reach, no board of its universe reaches; the reason is the mirror's."""
    cannot = tc.unreachable(v)
    other = {f for f in cannot if not f.startswith("steady")}
    assert other == ({"band<LV"} if v.lv == 1 else set()) | ({"middle-band-alone"} if v.fold else set())
    assert all(len(reason) > 20 for reason in cannot.values())
    for c in tc.universe(v):  # (every board up to the LDS capacity, at four of the depths)
        if c.K in (1, 4, 6, 13):
            assert not (tc.case_features(v, c) & set(cannot)), c


# ----- the plans -----

def _fold_lanes_repeat(waves):
    return all(np.array_equal(w.row0[:32], w.row0[32:]) and np.array_equal(w.col[:32], w.col[32:]) and
               np.array_equal(w.store[:32], w.store[32:]) for w in waves)


def _segments32(w):
    out, l = [], 0
    while l < 32:
        if w.store[l]:
            a = l
            while l < 32 and w.store[l] and w.row0[l] == w.row0[a] and w.col[l] == w.col[a] + (l - a):
                l += 1
            out.append((int(w.row0[a]), int(w.col[a]), l - a))
        else:
            l += 1
    return out


def plan_bands(waves, fold):
    segs = {(r0, w.nrows) for w in waves for r0, _, _ in (_segments32(w) if fold else wc.segments(w))}
    return sorted(segs)


def covers_once(waves, region, fold):
    r0, r1, c0, c1 = region
    n = np.zeros((r1 - r0, c1 - c0), np.int32)
    for w in waves:
        for sr, sc, sn in (_segments32(w) if fold else wc.segments(w)):
            n[sr - r0 : sr - r0 + w.nrows, sc - c0 : sc - c0 + sn] += 1
    return bool((n == 1).all())


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_sweep_plans(gol, v):
    """The tiles of the sweep's boards are the mirror's, at 192 columns and at the full-width shape of the family."""
    for W in (tc.COLS, tc.FULL_FOLD[0] if v.fold else wc.S3968.W):
        for c in tc.sweep_cases(v):
            nw = wc.nwords(W)
            waves, _ = tc.plan_tiles(gol, [(0, c.H, 0, nw)], W, c.H, c.rows, c.K, v.fold)
            assert plan_bands(waves, v.fold) == tc.tiles_of(c.H, c.rows)
            assert covers_once(waves, (0, c.H, 0, nw), v.fold)
            if v.fold:
                assert _fold_lanes_repeat(waves)
            if W == tc.FULL_FOLD[0]:  # 30 words: every folded band is one full 32-lane segment
                assert len(waves) == len(tc.tiles_of(c.H, c.rows))
                assert all(_segments32(w) == [(int(w.row0[0]), 0, tc.FOLD_SEG)] and not w.store[0] and not w.store[31]
                           for w in waves)
            if W == wc.S3968.W:
                assert all(wc.is_full_width(w) for w in waves) and len(waves) == len(tc.tiles_of(c.H, c.rows))


WIDE_FOLD_H, WIDE_FOLD_ROWS = 59, 30  # tiles of 30 and 29 rows: T even and odd at every depth


@pytest.mark.parametrize("K", tc.WIDE_DEPTHS)
def test_full_width_fold_plans(gol, K):
    """1920 columns: one full 32-lane segment per band.  2048: 30 + 2 words, the 2-word remainders packed."""
    H, rows = WIDE_FOLD_H, WIDE_FOLD_ROWS
    tiles = tc.tiles_of(H, rows)
    assert [n for _, n in tiles] == [30, 29]
    assert {tc.fold_geometry(n, K).odd for _, n in tiles} == {True, False}
    for W in tc.FULL_FOLD:
        nw = wc.nwords(W)
        waves, _ = tc.plan_tiles(gol, [(0, H, 0, nw)], W, H, rows, K, True)
        assert _fold_lanes_repeat(waves) and covers_once(waves, (0, H, 0, nw), True)
        assert plan_bands(waves, True) == tiles
        full = [w for w in waves if _segments32(w) == [(int(w.row0[0]), 0, tc.FOLD_SEG)]]
        assert len(full) == len(tiles)
        rest = [w for w in waves if w not in full]
        if W == 1920:
            assert not rest
        else:
            assert sorted(s for w in rest for s in _segments32(w)) == [(r0, tc.FOLD_SEG, 2) for r0, _ in tiles]
            assert all(int(w.store[:32].sum()) == 2 * len(_segments32(w)) for w in rest)


@pytest.mark.parametrize("K", tc.WIDE_DEPTHS)
@pytest.mark.parametrize("s", tc.WIDE, ids=wc.shape_id)
def test_wide_plain_plans(gol, s, K):
    """The wide shapes cut into two tiles keep what test_wide_plans.py pins for the rule kernels: per band the
    full-width segments (one row0, 62 words, the halo lanes 0 and 63), the tail word in lane 62 of a segment on 3950
    columns, packed remainders on 4096, a seam between full-width segments on 8000."""
    rows = wide_rows(s)
    nw = wc.nwords(s.W)
    waves, _ = tc.plan_tiles(gol, [(0, s.H, 0, nw)], s.W, s.H, rows, K, False)
    tiles = tc.tiles_of(s.H, rows)
    assert len(tiles) == 2 and plan_bands(waves, False) == tiles and covers_once(waves, (0, s.H, 0, nw), False)
    full = [w for w in waves if wc.is_full_width(w)]
    assert sorted((int(w.row0[0]), int(w.col[1])) for w in full) == [
        (r0, wc.SEG * i) for r0, _ in tiles for i in range(s.full_per_band)]
    rest = [seg for w in waves if not wc.is_full_width(w) for seg in wc.segments(w)]
    assert sorted(rest) == ([(r0, s.full_per_band * wc.SEG, s.rest) for r0, _ in tiles] if s.rest else [])
    if s is wc.S3950:
        assert all(int(w.col[62]) == nw - 1 and w.store[62] for w in full)
    if s is wc.S8000:  # the seam: segment 0's right halo lane streams word 62, which segment 1 stores
        assert any(int(w.col[1]) == 0 and int(w.col[63]) == wc.SEG for w in full)
    if s is wc.S4096 and tiles[0][1] == tiles[1][1]:
        assert any(wc.is_packed(w) for w in waves)


def wide_rows(s):
    return (s.H + 1) // 2


@pytest.mark.parametrize("K", tc.SPLIT_DEPTHS)
@pytest.mark.parametrize("H,W", tc.SPLIT_BOARDS)
def test_split_plans(gol, H, W, K):
    """A split superstep's interior folds; its bands of K rows never do (a folded plan needs a region of 28 rows),
    and each band is one tile."""
    nw = wc.nwords(W)
    interior, bands = tc.split_regions(H, nw, K)
    assert tc.folds([r[1] - r[0] for r in interior], tc.SPLIT_ROWS)
    assert not tc.folds([r[1] - r[0] for r in bands], tc.SPLIT_ROWS)
    waves, _ = tc.plan_tiles(gol, interior, W, H, tc.SPLIT_ROWS, K, True)
    assert _fold_lanes_repeat(waves)
    assert plan_bands(waves, True) == [(K + r0, n) for r0, n in tc.tiles_of(H - 2 * K, tc.SPLIT_ROWS)]
    assert all(tc.FOLD_MIN_ROWS // 2 <= n <= tc.SPLIT_ROWS for _, n in plan_bands(waves, True))
    waves, _ = tc.plan_tiles(gol, bands, W, H, tc.SPLIT_ROWS, K, False)
    assert plan_bands(waves, False) == [(0, K), (H - K, K)]


def test_phase_board():
    """Every 3 x 3 neighbourhood centred on rows of every phase mod 3, in even and in odd columns."""
    b = tc.phase_board()
    assert b.shape[0] % 3 == 0 and b.shape[1] == tc.COLS and b.shape[0] <= 300
    seen = tc.neighbourhoods_seen(b)
    assert all(seen[ph][par] == set(range(512)) for ph in range(3) for par in range(2))


def test_report():
    ref = np.zeros((60, 192), np.uint8)
    got = ref.copy()
    assert tc.tile_report(got, ref, 4, [(0, 30), (30, 30)]) == ""
    got[31, 70] = 1
    rep = tc.tile_report(got, ref, 4, [(0, 30), (30, 30)], fold=True, seg=tc.FOLD_SEG)
    assert "1 of 11520 cells differ" in rep and "row 31, column 70 = word 1" in rep
    assert "tile 1 of 2: rows 30 .. 59; tile row 1, in its first 4 rows" in rep
    assert "T = 38 (even), staged row 5 of half 0, 13.5 rows from the middle" in rep
