"""The plans of the wide boards of wide_cases.py, read from the lane descriptors of ``build_plan`` with the HIP
engine's arguments (region ``(0, H, 0, nw)``, segments of ``2K`` rows, x-wrap by the plan on an aligned torus): each
shape gives the plan feature test_gpu_wide.py relies on -- full-width waves with one ``row0``, packed remainders,
seams, the tail word's lane -- so a planner change cannot silently turn those tests into narrow-segment tests.  No
GPU is needed: the planner is host code.

Also here: the CPU backend, the GPU tests' second oracle, bit for bit against numpy at these widths."""
import numpy as np
import pytest

import wide_cases as wc
from wide_cases import DEPTHS, SEG, SHAPES, shape_id


def _plan(gol, s, K, boundary, rows_per_wave=0):
    waves, stats = wc.build(gol, s.H, s.W, K, boundary, rows_per_wave)
    return waves, stats


@pytest.mark.parametrize("boundary", wc.BOUNDARIES)
@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_shape_gives_its_feature(gol, s, K, boundary):
    nw = wc.nwords(s.W)
    assert nw == s.full_per_band * SEG + s.rest and s.W - 64 * (nw - 1) == s.tail_cells
    waves, stats = _plan(gol, s, K, boundary)
    assert wc.covers_once(waves, (0, s.H, 0, nw))
    bands = wc.bands_of(waves)
    assert bands == wc.equal_rows_bands(s.H, 2 * K) and all(K < n <= 2 * K for _, n in bands)
    assert stats["waves"] % 4 == 0 and stats["waves"] >= len(waves)

    full = [w for w in waves if wc.is_full_width(w)]
    rest = [w for w in waves if not wc.is_full_width(w)]
    # every band: its full-width segments, one wave each, at words 0, 62, ...
    assert sorted((int(w.row0[0]), int(w.col[1])) for w in full) == [
        (r0, SEG * i) for r0, _ in bands for i in range(s.full_per_band)]
    wrap = wc.xwrap(s.W, boundary)
    for w in full:
        c0 = int(w.col[1])
        assert w.col[1:63].tolist() == list(range(c0, c0 + SEG)) and not w.store[0] and not w.store[63]
        # halo lanes 0 and 63: the torus x-wrap by the plan, a ghost word, or (a seam) a word another wave stores
        left, right = int(w.col[0]), int(w.col[63])
        assert left == (c0 - 1 if c0 > 0 else (nw - 1 if wrap else -1))
        assert right == (c0 + SEG if c0 + SEG < nw else (0 if wrap else nw))
    # the row's remainder: one narrow segment per band, packed beside those of other bands
    if s.rest == 0:
        assert not rest
    else:
        segs = [seg for w in rest for seg in wc.segments(w)]
        assert sorted(segs) == [(r0, s.full_per_band * SEG, s.rest) for r0, _ in bands]
        by_height = {}
        for _, n in bands:
            by_height[n] = by_height.get(n, 0) + 1
        assert len(rest) == sum(-(-cnt // (64 // (s.rest + 2))) for cnt in by_height.values())
        if max(by_height.values()) >= 2:
            assert any(wc.is_packed(w) for w in rest)
        for w in rest:  # idle lanes stream an in-bounds word and never store
            assert int(w.store.sum()) == s.rest * len(wc.segments(w)) and w.col.min() >= -1 and w.col.max() <= nw
    # a seam between segments of one row: the halo lane streams an interior word that another wave owns
    if s.full_per_band * SEG < nw or s.full_per_band > 1:
        seam = SEG
        for r0, _ in bands:
            left_wave = [w for w in full if int(w.row0[0]) == r0 and int(w.col[1]) == 0]
            owners = [w for w in waves if any(sr == r0 and sc <= seam < sc + sn for sr, sc, sn in wc.segments(w))]
            assert len(left_wave) == 1 and len(owners) == 1 and owners[0].index != left_wave[0].index
            assert int(left_wave[0].col[63]) == seam and 0 < seam < nw
    # the tail word's place
    if s.tail_cells < 64:
        owner = [(w, seg) for w in waves for seg in wc.segments(w) if seg[1] <= nw - 1 < seg[1] + seg[2]]
        assert len(owner) == len(bands)
        for w, (_, sc, sn) in owner:
            if s.rest == 0:
                assert wc.is_full_width(w) and int(w.col[62]) == nw - 1  # lane 62 of a full-width segment
            else:
                assert (sc, sn) == (nw - 1, 1)  # a one-word segment of its own


def test_table_as_a_whole(gol):
    """What the table must provide somewhere: a full-width wave below row 0 and one that ends at the bottom edge (the
    scalar row masks with row0 != 0 and the owned-row span at the bottom), and a packed wave of one-word segments."""
    below = bottom = one_word_packed = False
    for s in SHAPES:
        for K in DEPTHS:
            waves, _ = _plan(gol, s, K, "dead")
            for w in waves:
                if wc.is_full_width(w):
                    below = below or int(w.row0[0]) > 0
                    bottom = bottom or int(w.row0[0]) + w.nrows == s.H
                elif wc.is_packed(w) and all(sn == 1 for _, _, sn in wc.segments(w)) and len(wc.segments(w)) >= 2:
                    one_word_packed = True
    assert below and bottom and one_word_packed


def test_loop_tail_set(gol):
    """Two bands of 21/20, 23/22, 25/24 rows: every residue of nrows mod 6 (and so of the kernels' row iterations
    n = nrows + 2K mod 6 for every K); the second band is full width, has row0 > 0 and ends at row H.  The tall case
    is two bands of 300."""
    residues = set()
    for H, heights in zip(wc.TAIL_HEIGHTS, [(21, 20), (23, 22), (25, 24)]):
        s = wc.tail_shape(H)
        for K in DEPTHS:
            for boundary in wc.BOUNDARIES:
                waves, _ = _plan(gol, s, K, boundary, wc.tail_rows(H))
                assert wc.bands_of(waves) == [(0, heights[0]), (heights[0], heights[1])]
                full = [w for w in waves if wc.is_full_width(w)]
                assert sorted(int(w.row0[0]) for w in full) == [0, heights[0]]
                assert any(int(w.row0[0]) > 0 and int(w.row0[0]) + w.nrows == H for w in full)
                assert len(waves) == 4  # (the two 2-word remainders differ in height: a wave each)
                residues |= {w.nrows % 6 for w in full}
                for K2 in DEPTHS:
                    assert {(w.nrows + 2 * K2) % 6 for w in full} == {(h + 2 * K2) % 6 for h in heights}
    assert residues == {0, 1, 2, 3, 4, 5}
    for K in wc.TALL_DEPTHS:
        waves, _ = _plan(gol, wc.TALL, K, "torus", wc.TALL_ROWS)
        assert wc.bands_of(waves) == [(0, 300), (300, 300)]
        assert sum(wc.is_full_width(w) for w in waves) == 2


def test_rank_plans_have_ghost_regions(gol):
    """The first pass of a two-pass superstep on a rank with neighbours: 1-D strips of 48 x 4096 extend 8 rows into the
    ghost rows; 2 x 2 tiles of 48 x 4096 also store the ghost words, a 66-word region cut 62 + 4."""
    waves, _ = wc.build(gol, 48, 4096, 8, "torus", region=(-8, 56, 0, 64))
    assert wc.bands_of(waves) == [(-8, 16), (8, 16), (24, 16), (40, 16)]
    assert sum(wc.is_full_width(w) for w in waves) == 4
    waves, _ = wc.build(gol, 48, 4096, 8, "dead", region=(-8, 56, -1, 65))
    assert wc.covers_once(waves, (-8, 56, -1, 65))
    full = [w for w in waves if wc.is_full_width(w)]
    assert len(full) == 4 and all(int(w.col[1]) == -1 and int(w.col[0]) == -1 for w in full)
    segs = sorted(seg for w in waves if not wc.is_full_width(w) for seg in wc.segments(w))
    assert segs == [(r0, 61, 4) for r0 in (-8, 8, 24, 40)]


def test_report_names_segment_lane_and_band_edge():
    """The failure report on a board with known wrong cells."""
    ref = np.zeros((48, 8000), np.uint8)
    assert wc.mismatch_report(ref, ref, 8, [(0, 16), (16, 16), (32, 16)]) == ""
    got = ref.copy()
    got[17, 64 * 70 + 5] = 1  # word 70: segment 1, lane 9; row 17 is the second row of band 16..31
    got[40, 64 * 124] = 1
    rep = wc.mismatch_report(got, ref, 8, [(0, 16), (16, 16), (32, 16)])
    assert rep.startswith("2 of 384000 cells differ")
    assert "row 17, column 4485 = word 70, segment 1, lane 9 of its segment; band rows 16..31, in its first 8 rows" in rep
    assert "wrong cells per segment: 1: 1, 2: 1" in rep and "2 wrong rows, 2 of them in the first / last 8 rows" in rep
    got = ref.copy()
    got[24, 0] = 1
    assert "segment 0, lane 1 of its segment; band rows 16..31, in its last 8 rows" in wc.mismatch_report(
        got, ref, 8, [(0, 16), (16, 16), (32, 16)])
    got = ref.copy()
    got[20, 3] = 1
    assert "inside" in wc.mismatch_report(got, ref, 4, [(0, 16), (16, 16), (32, 16)])


# ----- the CPU backend at these widths -----

CPU_SHAPES = SHAPES + [wc.tail_shape(H) for H in wc.TAIL_HEIGHTS]


@pytest.mark.parametrize("boundary", wc.BOUNDARIES)
@pytest.mark.parametrize("s", CPU_SHAPES, ids=shape_id)
def test_cpu_backend_matches_numpy(gol, s, boundary):
    """HighLife, 17 generations in supersteps of 8: the board against numpy_step_rule / numpy_step_rule_bounded, the
    census series against numpy_census."""
    gens = wc.SWEEP_GENS
    counts, boards = wc.history(s.H, s.W, wc.HIGHLIFE, boundary, gens)
    sim = gol.Simulation(s.H, backend="cpu", width=s.W, rule=wc.HIGHLIFE, boundary=boundary, halo_depth=8, census=True)
    sim.init(5, seed=wc.SEED)
    assert np.array_equal(sim.board(), wc.start_board(s.H, s.W))
    sim.step(gens)
    wc.check_census(sim, counts, boards[gens], 8, wc.equal_rows_bands(s.H, 16))
    assert wc.told_apart(s, gens)
    plain = gol.Simulation(s.H, backend="cpu", width=s.W, rule=wc.HIGHLIFE, boundary=boundary, halo_depth=8)
    plain.init(5, seed=wc.SEED).step(gens)
    wc.check_board(plain.board(), boards[gens], 8, wc.equal_rows_bands(s.H, 16))
