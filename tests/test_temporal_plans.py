"""The plans test_gpu_temporal.py relies on, read from ``build_plan`` with the HIP engine's arguments: the wide shapes
at depths 12 and 16 (test_wide_plans.py stops at 8), the loop-tail boards and the thread-rank strips at all ten
step_temporal depths, and the sub-tile halves of temporal_cases.SEAM_HEIGHTS, whose band heights must reach every
residue mod 6 (every height K .. 2K where K <= 4).  No GPU is needed: the planner is host code.  If an assertion
here fails, the shape is wrong for what the GPU test claims, not the assertion."""
import pytest

import temporal_cases as tc
import test_wide_plans as twp
import wide_cases as wc
from temporal_cases import TEMPORAL_DEPTHS
from wide_cases import SEG, SHAPES, shape_id

DEEP = [12, 16]


@pytest.mark.parametrize("K", DEEP)
@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_wide_shape_gives_its_feature_at_deep_depths(gol, s, K):
    """Full-width waves with one row0, the halo lanes' words, the seam, the tail word's lane and the packed remainders:
    the assertions of test_wide_plans.py, at the two depths only step_temporal has."""
    twp.test_shape_gives_its_feature(gol, s, K, "torus")
    waves, _ = wc.build(gol, s.H, s.W, K)
    full = [w for w in waves if wc.is_full_width(w)]
    assert len(wc.bands_of(waves)) >= 2  # (a band with row0 > 0, one that ends at the bottom edge)
    assert any(int(w.row0[0]) > 0 and int(w.row0[0]) + w.nrows == s.H for w in full)


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
def test_loop_tail_boards(gol, K):
    """One rank (region: the tile) and a thread-rank strip (the same region, no y-wrap): two full-width bands of
    21/20, 23/22, 25/24 rows, every residue of nrows mod 6 and so of the row iterations n = nrows + 2K."""
    residues = set()
    for H, heights in zip(wc.TAIL_HEIGHTS, [(21, 20), (23, 22), (25, 24)]):
        for region in (None, (0, H, 0, wc.nwords(wc.TAIL_W))):
            waves, _ = wc.build(gol, H, wc.TAIL_W, K, "torus", wc.tail_rows(H), region)
            assert wc.bands_of(waves) == [(0, heights[0]), (heights[0], heights[1])]
            full = [w for w in waves if wc.is_full_width(w)]
            assert sorted((int(w.row0[0]), w.nrows) for w in full) == [(0, heights[0]), (heights[0], heights[1])]
            residues |= {(w.nrows + 2 * K) % 6 for w in full}
    assert residues == {0, 1, 2, 3, 4, 5}
    assert [2 * H for H in wc.TAIL_HEIGHTS] == tc.GHOST_TAIL_HEIGHTS


@pytest.mark.parametrize("K", tc.TALL_DEPTHS)
def test_tall_board(gol, K):
    waves, _ = wc.build(gol, wc.TALL.H, wc.TALL.W, K, "torus", wc.TALL_ROWS)
    assert wc.bands_of(waves) == [(0, 300), (300, 300)]
    assert sum(wc.is_full_width(w) for w in waves) == 2


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
def test_multipass_rank_plans(gol, K):
    """The first pass of a two-pass superstep on a 48 x 4096 strip stores K ghost rows each side; on a 2 x 2 tile also
    the ghost words, a 66-word region cut 62 + 4."""
    h, nw = 48, 64
    assert 2 * K <= h  # (clamp_halo_depth: the halo fits the strip)
    region = (-K, h + K, 0, nw)
    waves, _ = wc.build(gol, h, 4096, K, "torus", region=region)
    assert wc.covers_once(waves, region)
    bands = wc.bands_of(waves)
    assert bands[0][0] == -K and bands[-1][0] + bands[-1][1] == h + K
    assert sum(wc.is_full_width(w) for w in waves) == len(bands)
    if K in tc.GRID_DEPTHS:
        region = (-K, h + K, -1, nw + 1)
        waves, _ = wc.build(gol, h, 4096, K, "torus", region=region, x_wrap=False)
        assert wc.covers_once(waves, region)
        full = [w for w in waves if wc.is_full_width(w)]
        assert len(full) == len(bands) and all(int(w.col[1]) == -1 and int(w.col[0]) == -1 for w in full)
        segs = sorted(seg for w in waves if not wc.is_full_width(w) for seg in wc.segments(w))
        assert segs == [(r0, SEG - 1, 4) for r0, _ in bands]


# ----- sub-tiles -----

@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
def test_seam_heights_cover_the_band_heights(gol, K):
    heights = tc.SEAM_HEIGHTS[K]
    assert len(heights) >= 3 and any(h >= 16 * K for h in heights)
    seen = set()
    for h in heights:
        assert h >= 8 * K
        for W in tc.SEAM_WIDTHS:
            assert W % 64 == 0
            for r0, hs in tc.sub_halves(h, K):
                assert hs >= K  # the other half reads K edge rows of this one
                rows = tc.sub_rows(gol, hs, W, K, 0, tc.RESIDENT_MIN)
                assert rows == tc.sub_rows(gol, hs, W, K, 0, tc.RESIDENT_MAX) == min(2 * K, hs)
                _, waves, _ = tc.sub_build(gol, hs, W, K)
                assert wc.covers_once(waves, tc.sub_region(hs, wc.nwords(W), 0))
                bands = wc.bands_of(waves)
                assert bands[0][0] == 0 and bands[-1][0] + bands[-1][1] == hs  # the source switches at rows 0 and h
                assert all(K <= n <= 2 * K for _, n in bands)
                seen |= {n for _, n in bands}
    if K >= 5:
        assert {n % 6 for n in seen} == {0, 1, 2, 3, 4, 5}, sorted(seen)
    else:  # every height a sub-tile plan of this depth can have
        assert seen == set(range(K, 2 * K + 1)), sorted(seen)


@pytest.mark.parametrize("W,full_per_band,rest", [(3968, 1, 0), (8192, 2, 4), (192, 0, 3)])
def test_seam_widths_give_their_segments(gol, W, full_per_band, rest):
    """3968: each band one full-width segment with the x-wrap in lanes 0 and 63; 8192: a seam between two full-width
    segments and a packed remainder; 192: narrow packed segments only."""
    nw = wc.nwords(W)
    assert nw == full_per_band * SEG + rest
    for K in TEMPORAL_DEPTHS:
        for h in tc.SEAM_HEIGHTS[K]:
            for _, hs in tc.sub_halves(h, K):
                _, waves, _ = tc.sub_build(gol, hs, W, K)
                bands = wc.bands_of(waves)
                full = [w for w in waves if wc.is_full_width(w)]
                assert sorted((int(w.row0[0]), int(w.col[1])) for w in full) == [
                    (r0, SEG * i) for r0, _ in bands for i in range(full_per_band)]
                for w in full:
                    c0 = int(w.col[1])
                    assert int(w.col[0]) == (c0 - 1 if c0 > 0 else nw - 1)
                    assert int(w.col[63]) == (c0 + SEG if c0 + SEG < nw else 0)
                segs = sorted(seg for w in waves if not wc.is_full_width(w) for seg in wc.segments(w))
                assert segs == ([(r0, full_per_band * SEG, rest) for r0, _ in bands] if rest else [])


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
def test_seam_then_ghost_heights(gol, K):
    """halo_depth = 2K: the seam pass stores K ghost rows each side of a half, the ghost pass the half's own rows."""
    R, W = 2 * K, tc.SEAM2_WIDTH
    for h in tc.seam2_heights(K):
        assert h >= 8 * R
        for _, hs in tc.sub_halves(h, R):
            assert hs >= R
            for e in (K, 0):
                assert tc.sub_rows(gol, hs, W, K, e, tc.RESIDENT_MIN) == tc.sub_rows(gol, hs, W, K, e, tc.RESIDENT_MAX) == 2 * K
                _, waves, _ = tc.sub_build(gol, hs, W, K, e)
                assert wc.covers_once(waves, tc.sub_region(hs, wc.nwords(W), e))
                assert any(wc.is_full_width(w) for w in waves) and any(not wc.is_full_width(w) for w in waves)
    assert tc.sub_halves(tc.seam2_heights(K)[0], R) == [(0, 16 * K), (16 * K, 2 * K + 1)]


def test_cuts_and_entries():
    assert tc.cut(8, 8) == "cut8=temporal@8" and tc.cut(24, 12) == "cut24=temporal@12+temporal@12"
    assert tc.sub_entries(16, 1, [(16, 12)]) == ["sub16.1.0=16rows,12waves"]
    assert tc.sub_entries(24, 0, [(8, 4), (8, 4), (8, 8)]) == ["sub24.0.0-1=8rows,4waves", "sub24.0.2=8rows,8waves"]
    assert tc.sub_halves(640, 8) == [(0, 320), (320, 320)] and tc.sub_halves(73, 8) == [(0, 64), (64, 9)]
    assert all(K <= N for N, K in tc.SIZE_CASES) and len(tc.SIZE_CASES) == 76
