"""step_pipe<NW, L, WRAPY> (csrc/src/hip/pipe_kernel.hip) in all 48 instantiations -- NW in {5, 7, 9, 11, 13, 16} waves
x L in {1, 2, 3, 4} generations per stage x STEP_WRAP_Y on / off -- bit for bit against numpy (B3/S23 on the torus),
on the boards of pipe_cases.py; test_pipe_plans.py asserts on the CPU that those boards contain what is claimed here.

Every run is pinned: GOL_PIPE names the geometry (one workgroup per CU) and kernel_depth = K = (NW - 1) L keeps the
engine from measuring pass costs, so a pass of K generations can only be step_pipe in that geometry.  Nothing about
what ran is assumed all the same: before a board is compared the test asserts the kernel, its depth, the superstep's
``cut<R>=pipe@K((NW-1)xL,1/CU)`` entry of stats()["tuning"] and that the engine's plan has the waves and the bands
``build_plan`` gives for the same arguments.  Unless it says otherwise a test runs 2K + 1 generations: two step_pipe
supersteps and a one-generation step_temporal remainder.  A wrong board fails with wide_cases.mismatch_report.

  * STEP_WRAP_Y, one rank:    every branch of ``stage`` in each role and every path of the loader (the loop-tail
                              boards), the wide shapes (full-width segments and their seam, ghost words, the tail word
                              in lane 62, one-word tail segments, the x-wrap across two waves), boards of exactly K and
                              K + 1 rows at 64, 65 and 128 columns, 300-row segments;
  * ghost rows, thread ranks: strips whose loader reuses no ring slot, ordinary ones and bands of more than 40 rows;
                              supersteps of two passes (the first stores the ghost rows the second reads); a 2 x 2 grid
                              (ghost words stored too).

The split schedule (its interior kernel is chosen by timing, so it cannot be pinned) is not covered here; the resident
kernel has its own every-variant file, test_gpu_resident_variants.py."""
import pytest

import pipe_cases as pc
import wide_cases as wc
from pipe_cases import GEOMETRIES, gid
from wide_cases import shape_id

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_spinup(monkeypatch):
    monkeypatch.setenv("GOL_SPINUP_MS", "0")


def check_ran(gol, stats, H, W, nw, L, R, schedule, rows_per_wave, region=None, x_wrap=None):
    """step_pipe in geometry (nw, L) at one workgroup per CU, in supersteps of R generations cut into passes of K, on
    the plan ``build_plan`` gives for the same arguments; returns that plan's row bands."""
    K = pc.depth(nw, L)
    assert stats["kernel"] == pc.kernel_name(nw, L), stats
    assert stats["kernel_depth"] == K and stats["depth"] == R and stats["schedule"] == schedule, stats
    assert pc.cut(R, nw, L) in stats["tuning"].split(), stats["tuning"]
    waves, pst = wc.build(gol, H, W, K, "torus", rows_per_wave, region, x_wrap)
    assert stats["plan_waves"] == pst["waves"], (stats["plan_waves"], pst)
    return wc.bands_of(waves)


# ----- 1. STEP_WRAP_Y: one rank -----

def run_pipe(gol, monkeypatch, H, W, nw, L, rows_per_wave, gens=None, total=pc.GENS_TOTAL):
    assert rows_per_wave > 0
    K = pc.depth(nw, L)
    gens = pc.gens_of(K) if gens is None else gens
    monkeypatch.setenv("GOL_PIPE", f"{nw},{L},1")
    monkeypatch.setenv("GOL_SPINUP_MS", "0")
    sim = gol.Simulation(H, backend="hip", device=0, width=W, kernel="pipe", kernel_depth=K, halo_depth=K, subtiles=0,
                         rows_per_wave=rows_per_wave).init(5, seed=wc.SEED)
    bands = check_ran(gol, sim.stats(), H, W, nw, L, K, "local", rows_per_wave)
    assert bands == wc.equal_rows_bands(H, rows_per_wave), bands
    sim.step(gens)
    wc.check_board(sim.board(), pc.conway_after(H, W, gens, total), K, bands)


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_wrap_loop_tails(gol, monkeypatch, g):
    """pipe_cases.loop_tail_cases: per role the fill's early return, the partly filled queue, zero, one and more steady
    turns, every count of rows left at the tail, the second tail pass, the four refills; the loader with 12 rows or
    fewer, without and with slot reuse, as a single, top, middle and bottom band."""
    for c in pc.loop_tail_cases(*g):
        run_pipe(gol, monkeypatch, c.H, wc.TAIL_W, *g, c.rows)


@pytest.mark.parametrize("s,g", [(s, g) for g in GEOMETRIES for s in pc.wide_cases(*g)],
                         ids=lambda v: shape_id(v) if isinstance(v, wc.Shape) else gid(v))
def test_wrap_wide(gol, monkeypatch, s, g):
    """The wide shapes of at least K rows in two bands: unaligned widths (ghost words, the tail word in lane 62, a
    one-cell tail word), the seam between two full-width segments, the x-wrap across two waves."""
    run_pipe(gol, monkeypatch, s.H, s.W, *g, pc.wide_rows(s))


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_wrap_small_boards(gol, monkeypatch, g):
    """Boards of exactly K rows (the stream is the board three times over) and of K + 1, at 64 columns (the one word is
    its own neighbour), 65 (a one-cell tail word) and 128; as a single band and as bands of one row."""
    for c in pc.small_cases(*g):
        run_pipe(gol, monkeypatch, c.H, c.W, *g, c.rows)


@pytest.mark.parametrize("g", pc.TALL_GEOMETRIES, ids=gid)
def test_wrap_tall_segments(gol, monkeypatch, g):
    """Two bands of 300 rows: many turns of every stage's steady loop."""
    run_pipe(gol, monkeypatch, wc.TALL.H, wc.TALL.W, *g, wc.TALL_ROWS, total=wc.TALL_GENS)


# ----- 2. ghost rows: thread ranks sharing the GPU -----

def run_ghost(gol, monkeypatch, P, s, nw, L, R, gens, tile, region, rows_per_wave, x_wrap=None, **kw):
    """A global board ``s`` on P thread ranks with tiles ``tile`` = (h, w), schedule "full": every pass reads ghost
    rows (no STEP_WRAP_Y); the assembled board against numpy."""
    K = pc.depth(nw, L)
    monkeypatch.setenv("GOL_PIPE", f"{nw},{L},1")  # (in the parent, before the rank threads start)
    monkeypatch.setenv("GOL_SPINUP_MS", "0")

    def script(sim):
        sim.step(gens)

    parts = wc.run_ranks(gol, P, s.H, s.W, "hip", script, halo_depth=R, kernel_depth=K, kernel="pipe", schedule="full",
                         subtiles=0, rows_per_wave=rows_per_wave, **kw)
    want = [(r0 + region[0], n) for r0, n in wc.equal_rows_bands(region[1] - region[0], rows_per_wave)]
    for p in parts:
        assert p.board.shape == tile, (p.rank, p.board.shape)
        bands = check_ran(gol, p.stats, tile[0], tile[1], nw, L, R, "full", rows_per_wave, region, x_wrap)
        assert bands == want, (p.rank, bands)
    wc.check_ranks(s.H, s.W, parts, pc.conway_after(s.H, s.W, gens), bands, K)


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_ghost_loop_tails(gol, monkeypatch, g):
    """P = 2, one pass per superstep, pipe_cases.ghost_strips: the loader's paths again, reading ghost rows."""
    K = pc.depth(*g)
    for st in pc.ghost_strips(*g):
        run_ghost(gol, monkeypatch, 2, wc.Shape(2 * st.h, wc.TAIL_W, 1, 2, 64), *g, K, pc.gens_of(K), (st.h, wc.TAIL_W),
                  (0, st.h, 0, wc.nwords(wc.TAIL_W)), st.rows)


@pytest.mark.parametrize("g", pc.MULTI_GEOMETRIES, ids=gid)
def test_ghost_multipass(gol, monkeypatch, g):
    """P = 2 on 96 x 4096, supersteps of two passes of K: the first stores K ghost rows each side, the second reads
    them; 4K + 3 generations."""
    K, s = pc.depth(*g), pc.MULTI
    h = s.H // 2
    run_ghost(gol, monkeypatch, 2, s, *g, 2 * K, 4 * K + 3, (h, s.W), (-K, h + K, 0, wc.nwords(s.W)), pc.MULTI_ROWS)


@pytest.mark.parametrize("g", pc.GRID_GEOMETRIES, ids=gid)
def test_ghost_grid(gol, monkeypatch, g):
    """2 x 2 on 96 x 8192: the first pass also stores the ghost words, a 66-word region cut 62 + 4."""
    K, s = pc.depth(*g), pc.GRID
    h, w = s.H // 2, s.W // 2
    run_ghost(gol, monkeypatch, 4, s, *g, 2 * K, 4 * K + 3, (h, w), (-K, h + K, -1, wc.nwords(w) + 1), pc.MULTI_ROWS,
              x_wrap=False, decomp="2d", grid="2x2")
