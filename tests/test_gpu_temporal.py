"""step_temporal<K, ROWS>, the kernel the headline numbers come from, at each of its ten depths (1 .. 8, 12, 16) in
each of its three row modes, bit for bit against numpy (B3/S23 on the torus):

  * ROWS_WRAP   one rank: the wide shapes of wide_cases.py (full-width segments, the tail word in lane 62, a one-word
                masked tail segment, a seam between full-width segments, the x-wrap across two waves; the unaligned
                widths stream ghost words), every tail of the steady loops (bands of 20 .. 25 rows), 300-row segments,
                the ten board sizes (on 1, 2 and 3 rows the load row wraps several times per pass);
  * ROWS_GHOST  thread ranks sharing the GPU: the loop tails again (K = 5 is the two-triple loop only this mode has),
                supersteps of two passes (the first stores the ghost rows the second reads), a 2 x 2 grid (ghost words
                stored, 66-word regions cut 62 + 4);
  * ROWS_SEAM   two sub-tiles: one seam pass per superstep over halves whose band heights are every residue mod 6
                (test_temporal_plans.py asserts it), then a seam pass followed by a ghost pass;

and word for word against step_rule<K> under B3/S23, whose runner is separate.

Nothing about what ran is assumed: every test asserts the kernel, its depth, the superstep's cut and that the engine's
plan has the waves ``build_plan`` gives for the same arguments; the sub-tile tests read the halves' plans from
stats()["tuning"].  A wrong board fails with wide_cases.mismatch_report."""
import numpy as np
import pytest

import temporal_cases as tc
import wide_cases as wc
from temporal_cases import TEMPORAL_DEPTHS
from wide_cases import CONWAY, SHAPES, shape_id

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_spinup(monkeypatch):
    monkeypatch.setenv("GOL_SPINUP_MS", "0")


def check_ran(gol, stats, H, W, K, R, schedule, rows_per_wave=0, region=None, x_wrap=None):
    """step_temporal at depth K in supersteps of R generations cut into passes of K, under ``schedule``, on the plan
    ``build_plan`` gives for the same arguments; returns that plan's row bands."""
    assert stats["kernel"] == "temporal" and stats["kernel_depth"] == K and stats["depth"] == R, stats
    assert stats["schedule"] == schedule, stats
    assert tc.cut(R, K) in stats["tuning"].split(), stats["tuning"]
    waves, pst = wc.build(gol, H, W, K, "torus", rows_per_wave, region, x_wrap)
    assert stats["plan_waves"] == pst["waves"], (stats["plan_waves"], pst)
    return wc.bands_of(waves)


# ----- 1. ROWS_WRAP: one rank -----

def run_wrap(gol, H, W, K, gens, total, rows_per_wave=0, want_bands=None):
    sim = gol.Simulation(H, backend="hip", device=0, width=W, kernel="temporal", kernel_depth=K, halo_depth=K,
                         subtiles=0, rows_per_wave=rows_per_wave).init(5, seed=wc.SEED)
    bands = check_ran(gol, sim.stats(), H, W, K, K, "local", rows_per_wave)
    assert want_bands is None or bands == want_bands, bands
    sim.step(gens)
    wc.check_board(sim.board(), tc.conway_after(H, W, gens, total), K, bands)


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_wrap_wide_sweep(gol, s, K):
    """2K + 1 generations: two one-pass supersteps of depth K and a remainder."""
    run_wrap(gol, s.H, s.W, K, tc.gens_of(K), tc.GENS_TOTAL)


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
@pytest.mark.parametrize("H", wc.TAIL_HEIGHTS)
def test_wrap_loop_tails(gol, H, K):
    """Two full-width bands of 21/20, 23/22, 25/24 rows: every residue of n = nrows + 2K mod 6, so the six-row loop
    of K <= 4, the two-triple loop of K = 6, 7, 12 with its leftover triple, and the 0-2 tail rows of every loop."""
    top = wc.tail_rows(H)
    run_wrap(gol, H, wc.TAIL_W, K, tc.gens_of(K), tc.GENS_TOTAL, top, [(0, top), (top, H - top)])


@pytest.mark.parametrize("K", tc.TALL_DEPTHS)
def test_wrap_tall_segments(gol, K):
    """Two bands of 300 rows: many iterations of the steady loop before its tail."""
    run_wrap(gol, wc.TALL.H, wc.TALL.W, K, wc.TALL_GENS, wc.TALL_GENS, wc.TALL_ROWS, [(0, 300), (300, 300)])


@pytest.mark.parametrize("N,K", tc.SIZE_CASES)
def test_wrap_board_sizes(gol, N, K):
    """The ten board sizes at every depth K <= N (the halo depth is clamped to the tile's rows)."""
    run_wrap(gol, N, N, K, tc.gens_of(K), tc.GENS_TOTAL)


# ----- 2. ROWS_GHOST: thread ranks sharing the GPU -----

def run_ghost(gol, P, s, K, R, gens, total, tile, region, rows_per_wave=0, want_bands=None, x_wrap=None, **kw):
    """A global board ``s`` on P thread ranks with tiles ``tile`` = (h, w), schedule "full": every pass has ghost rows
    (no STEP_WRAP_Y); the assembled board against numpy."""
    def script(sim):
        sim.step(gens)

    parts = wc.run_ranks(gol, P, s.H, s.W, "hip", script, halo_depth=R, kernel_depth=K,
                         kernel="temporal", schedule="full", subtiles=0, rows_per_wave=rows_per_wave, **kw)
    for p in parts:
        assert p.board.shape == tile, (p.rank, p.board.shape)
        bands = check_ran(gol, p.stats, tile[0], tile[1], K, R, "full", rows_per_wave, region, x_wrap)
        assert want_bands is None or bands == want_bands, (p.rank, bands)
    wc.check_ranks(s.H, s.W, parts, tc.conway_after(s.H, s.W, gens, total), bands, K)


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
@pytest.mark.parametrize("H", tc.GHOST_TAIL_HEIGHTS)
def test_ghost_loop_tails(gol, H, K):
    """P = 2, strips of 41, 45, 49 rows in two full-width bands, one pass per superstep: the loop tails of
    test_wrap_loop_tails with ghost rows; K = 5 is the two-triple loop that only ROWS_GHOST has."""
    h = H // 2
    top = wc.tail_rows(h)
    run_ghost(gol, 2, wc.Shape(H, wc.TAIL_W, 1, 2, 64), K, K, tc.gens_of(K), tc.GENS_TOTAL, (h, wc.TAIL_W),
              (0, h, 0, wc.nwords(wc.TAIL_W)), top, [(0, top), (top, h - top)])


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
def test_ghost_multipass(gol, K):
    """P = 2 on 96 x 4096, supersteps of two passes of K: the first stores K ghost rows each side, the second reads
    them; 4K + 3 generations."""
    s = tc.MULTI
    run_ghost(gol, 2, s, K, 2 * K, 4 * K + 3, tc.MULTI_GENS_TOTAL, (48, 4096), (-K, 48 + K, 0, 64))


@pytest.mark.parametrize("K", tc.GRID_DEPTHS)
def test_ghost_grid(gol, K):
    """2 x 2 on 96 x 8192: the first pass also stores the ghost words, a 66-word region cut 62 + 4."""
    s = tc.GRID
    run_ghost(gol, 4, s, K, 2 * K, 4 * K + 3, tc.MULTI_GENS_TOTAL, (48, 4096), (-K, 48 + K, -1, 65), x_wrap=False,
              decomp="2d", grid="2x2")


# ----- 3. ROWS_SEAM: two sub-tiles -----

def run_seam(gol, h, W, K, R, steps):
    """Two sub-tiles at pass depth K and halo depth R; ``steps``: the generations of each step() call."""
    sim = gol.Simulation(h, backend="hip", device=0, width=W, kernel="temporal", kernel_depth=K, halo_depth=R,
                         subtiles=2).init(5, seed=wc.SEED)
    st = sim.stats()
    assert "+subtiles2" in st["schedule"], st
    check_ran(gol, st, h, W, K, R, "local+subtiles2")
    # the halves' plans: pass j stores the ghost rows of the passes after it
    plans = [[], []]
    for j in range(R // K):
        bands, per_half = tc.sub_bands(gol, h, W, K, R, R - (j + 1) * K)
        for half in (0, 1):
            plans[half].append(per_half[half])
    got = [t for t in st["tuning"].split() if t.startswith("sub")]
    assert got == tc.sub_entries(R, 0, plans[0]) + tc.sub_entries(R, 1, plans[1]), (plans, st["tuning"])
    gens = sum(steps)
    for n in steps:
        sim.step(n)
    wc.check_board(sim.board(), tc.conway_after(h, W, gens, gens), K, bands)  # (the last pass's bands)


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
@pytest.mark.parametrize("W", tc.SEAM_WIDTHS)
def test_seam_pass(gol, W, K):
    """One seam pass per superstep, 3K + 1 generations in two step() calls, on halves whose bands are together every
    residue mod 6 (K <= 4: every height K .. 2K); each half's first band starts at row 0 and its last ends at row h,
    where the load stream switches sources."""
    for h in tc.SEAM_HEIGHTS[K]:
        run_seam(gol, h, W, K, K, [K + 1, 2 * K])


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
def test_seam_then_ghost_pass(gol, K):
    """halo_depth = 2K: a seam pass that stores the halves' ghost rows, then a ghost pass; two supersteps and a
    remainder rotate through the three buffers of each half."""
    for h in tc.seam2_heights(K):
        run_seam(gol, h, tc.SEAM2_WIDTH, K, 2 * K, [2 * K + 1, 2 * K + 2])


@pytest.mark.parametrize("K", TEMPORAL_DEPTHS)
def test_subtiles_refused_without_room_for_the_edge_rows(gol, K):
    """Tiles of 8K .. 9K - 1 rows would be cut into halves of 8K and fewer than K rows, and the first half's seam
    pass would read K edge rows of the second: the engine runs them as one tile (the shortest tile that is cut, 9K
    rows, is in SEAM_HEIGHTS for K <= 5)."""
    W, gens = tc.SEAM_WIDTHS[0], 3 * K + 1
    for h in sorted({8 * K, 9 * K - 1}):
        assert tc.sub_halves(h, K)[1][1] < K
        sim = gol.Simulation(h, backend="hip", device=0, width=W, kernel="temporal", kernel_depth=K, halo_depth=K,
                             subtiles=2).init(5, seed=wc.SEED)
        bands = check_ran(gol, sim.stats(), h, W, K, K, "local")
        sim.step(K + 1)
        sim.step(2 * K)
        wc.check_board(sim.board(), tc.conway_after(h, W, gens, gens), K, bands)


# ----- 4. against step_rule<K> -----

@pytest.mark.parametrize("K", wc.DEPTHS)
@pytest.mark.parametrize("s", tc.CROSS_SHAPES, ids=shape_id)
def test_against_generic_kernel(gol, s, K):
    """Two kernels with separate runners agree on every stored word, the masked tail word included."""
    gens = tc.gens_of(K)
    kw = dict(backend="hip", device=0, width=s.W, kernel_depth=K, halo_depth=K, subtiles=0)
    a = gol.Simulation(s.H, kernel="temporal", **kw).init(5, seed=wc.SEED)
    b = gol.Simulation(s.H, kernel="rule", rule=CONWAY, **kw).init(5, seed=wc.SEED)
    bands = check_ran(gol, a.stats(), s.H, s.W, K, K, "local")
    assert b.stats()["kernel"] == f"rule@{K}" and b.stats()["kernel_depth"] == K, b.stats()
    assert b.stats()["plan_waves"] == a.stats()["plan_waves"]
    a.step(gens)
    b.step(gens)
    wc.check_board(a.board(), tc.conway_after(s.H, s.W, gens, tc.GENS_TOTAL), K, bands)
    wa, wb = a.words(), b.words()
    assert wa.shape == wb.shape == (s.H, wc.nwords(s.W))
    assert np.array_equal(wa, wb), f"{int((wa != wb).sum())} words differ, first at {np.argwhere(wa != wb)[0].tolist()}"
