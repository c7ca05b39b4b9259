"""step_rule<K>, step_rule_bounded<K> and step_census<K> on boards wide enough for full-width segments (the shapes of
wide_cases.py, 3950 to 8192 columns), bit for bit against numpy.  The benchmarked boards are 8192 and 32768 columns
wide; the other tests of these kernels stop at 1000 columns, where a row band is one 18-lane segment and three
segments of different rows share a wave.  What runs only here:

  * a wave that is one 64-lane segment: lanes 0 and 63 are the halo lanes and stream the x-wrap words, the ghost words
    or (a seam) a word that another wave stores;
  * the scalar-mask runners of step_rule_bounded and step_census (one row0 per wave, A / Ao / ospan through
    readfirstlane) on full-width segments, with row0 != 0 and at the bottom edge (on narrow boards only a band whose
    height differs from the others', alone in its wave, takes them);
  * the row's remainder, and the masked tail word, as a narrow segment packed beside those of other bands;
  * every tail of the steady loops (two bands of 21/20, 23/22, 25/24 rows) and 300-row segments;
  * ROWS_GHOST passes over full-width segments, and 66-word regions (ghost words stored) cut 62 + 4.

Every test asserts the kernel and that the engine's plan has the wave count of the plan test_wide_plans.py inspects.
A wrong board fails with wide_cases.mismatch_report: wrong cells, the first one's row, word, segment and lane, and
whether its row lies in the first or last K rows of its band."""
import numpy as np
import pytest

import wide_cases as wc
from grid_cases import np_density
from wide_cases import B1, BOUNDARIES, CONWAY, DEPTHS, HIGHLIFE, RULES, S4096, S8000, SHAPES, shape_id

pytestmark = pytest.mark.gpu

KERNELS = ["rule", "bounded", "census"]


@pytest.fixture(autouse=True)
def _no_spinup(monkeypatch):
    monkeypatch.setenv("GOL_SPINUP_MS", "0")


def _sim(gol, s, K, rule, boundary, **kw):
    kw.setdefault("halo_depth", K)
    return gol.Simulation(s.H, backend="hip", device=0, width=s.W, rule=rule, boundary=boundary, kernel_depth=K,
                          subtiles=0, **kw).init(5, seed=wc.SEED)


def check_plan(gol, stats, s, K, boundary, census=False, rows_per_wave=0, region=None):
    """The kernel is the generic one at depth K and the engine's plan has as many waves as ``build_plan`` gives for the
    same arguments; returns that plan's row bands."""
    name = "census" if census else "rule"
    assert stats["kernel"].startswith(f"{name}@{K}") and stats["boundary"] == boundary, stats
    assert stats["census"] is census and stats["kernel_depth"] == K, stats
    waves, pst = wc.build(gol, s.H, s.W, K, boundary, rows_per_wave, region)
    assert stats["plan_waves"] == pst["waves"], (stats["plan_waves"], pst)
    return wc.bands_of(waves)


def run_kernel(gol, s, K, kernel, gens, total, rows_per_wave=0, want_bands=None, **kw):
    """``gens`` generations of one of the three kernels on shape ``s`` under its rules (census: under both boundaries),
    against the numpy history over ``total`` generations."""
    for boundary in {"rule": ["torus"], "bounded": ["dead"], "census": BOUNDARIES}[kernel]:
        for rule in RULES[boundary]:
            census = kernel == "census"
            sim = _sim(gol, s, K, rule, boundary, census=census, rows_per_wave=rows_per_wave, **kw)
            bands = check_plan(gol, sim.stats(), s, K, boundary, census, rows_per_wave)
            assert want_bands is None or bands == want_bands, bands
            sim.step(gens)
            ref = wc.board_after(s, rule, boundary, gens, total)
            if census:
                wc.check_census(sim, wc.counts_until(s, rule, boundary, gens, total), ref, K, bands)
            else:
                wc.check_board(sim.board(), ref, K, bands)
        if boundary == "dead":
            assert wc.told_apart(s, gens, total), "the input does not tell the boundaries apart"


# ----- 1. the sweep: every shape x depth x kernel on the default plan -----

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_sweep(gol, s, K, kernel):
    """2K + 1 generations: a superstep, a second one, a remainder."""
    run_kernel(gol, s, K, kernel, 2 * K + 1, wc.SWEEP_GENS)


# ----- 2. loop tails and tall segments -----

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("H", wc.TAIL_HEIGHTS)
def test_loop_tails(gol, H, K, kernel):
    """Two full-width bands of (H + 1) // 2 and H // 2 rows: 21/20, 23/22, 25/24 are every residue of the row
    iterations n = nrows + 2K mod 6; the second band has row0 > 0 and ends at the bottom edge."""
    top = wc.tail_rows(H)
    run_kernel(gol, wc.tail_shape(H), K, kernel, 2 * K + 1, wc.SWEEP_GENS, rows_per_wave=top,
               want_bands=[(0, top), (top, H - top)])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("K", wc.TALL_DEPTHS)
def test_tall_segments(gol, K, kernel):
    """Two bands of 300 rows: many iterations of the steady loop before its tail."""
    run_kernel(gol, wc.TALL, K, kernel, wc.TALL_GENS, wc.TALL_GENS, rows_per_wave=wc.TALL_ROWS,
               want_bands=[(0, 300), (300, 300)])


# ----- 3. multi-pass supersteps -----

@pytest.mark.parametrize("mode", ["rule-graph", "rule-eager", "bounded", "census"])
@pytest.mark.parametrize("R", [16, 24])
@pytest.mark.parametrize("s", [S4096, S8000], ids=shape_id)
def test_multipass_supersteps(gol, s, R, mode):
    """Supersteps of two and three passes of 8: later passes read what earlier ones wrote.  Bounded and census run
    eager; the torus kernel under a graph and without."""
    gens, K = 37, 8
    kernel, graph = mode.split("-")[0], mode == "rule-graph"
    for boundary in {"rule": ["torus"], "bounded": ["dead"], "census": BOUNDARIES}[kernel]:
        for rule in RULES[boundary]:
            census = kernel == "census"
            sim = _sim(gol, s, K, rule, boundary, census=census, halo_depth=R, graph=graph)
            st = sim.stats()
            assert st["depth"] == R, st
            bands = check_plan(gol, st, s, K, boundary, census)
            sim.step(gens)
            st = sim.stats()
            assert (st["graph_launches"] >= 1) if graph else (st["graph_launches"] == 0), st
            ref = wc.board_after(s, rule, boundary, gens, gens)
            if census:
                wc.check_census(sim, wc.counts_until(s, rule, boundary, gens, gens), ref, K, bands)
            else:
                wc.check_board(sim.board(), ref, K, bands)
        if boundary == "dead":
            assert wc.told_apart(s, gens, gens)


# ----- 4. B3/S23 through the generic kernel -----

@pytest.mark.parametrize("s", [S4096, S8000], ids=shape_id)
def test_conway_through_generic_kernel(gol, s):
    """Against numpy, and word for word against the specialised step_temporal on the same board."""
    gens, K = 17, 8
    a = _sim(gol, s, K, CONWAY, "torus", kernel="rule")
    b = _sim(gol, s, K, CONWAY, "torus", kernel="temporal")
    bands = check_plan(gol, a.stats(), s, K, "torus")
    assert b.stats()["kernel"].startswith("temporal"), b.stats()
    a.step(gens)
    b.step(gens)
    wc.check_board(a.board(), wc.board_after(s, CONWAY, "torus", gens, gens), K, bands)
    assert np.array_equal(a.words(), b.words())


# ----- 5. thread ranks: ROWS_GHOST passes over full-width segments -----

RANK_CONFIGS = {
    # P, global H x W, Simulation arguments, the first pass's region on a 48 x 4096 tile
    "P2-full": (2, 96, 4096, {"schedule": "full"}, (-8, 56, 0, 64)),
    "P2-split": (2, 96, 4096, {"schedule": "split"}, (-8, 56, 0, 64)),
    "2x2": (4, 96, 8192, {"decomp": "2d", "grid": "2x2"}, (-8, 56, -1, 65)),
}
RANK_RULE = {"torus": HIGHLIFE, "dead": B1}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("config", list(RANK_CONFIGS))
def test_thread_ranks(gol, config, kernel):
    """Strips and tiles of 48 x 4096 as thread ranks sharing the GPU, 40 generations in supersteps of two passes of 8:
    the earlier pass stores the ghost rows (in the grid the ghost words too, a 66-word region cut 62 + 4).  Against
    numpy on the assembled board and against the CPU backend on the same decomposition."""
    P, H, W, kw, region = RANK_CONFIGS[config]
    tile = wc.Shape(48, 4096, 1, 2, 64)
    census = kernel == "census"
    for boundary in {"rule": ["torus"], "bounded": ["dead"], "census": BOUNDARIES}[kernel]:
        rule = RANK_RULE[boundary]
        counts, boards = wc.history(H, W, rule, boundary, wc.RANK_GENS)
        ref = boards[wc.RANK_GENS]
        script = wc.census_script if census else None
        parts = wc.run_ranks(gol, P, H, W, "hip", script, rule=rule, boundary=boundary, census=census, **kw)
        for p in parts:
            assert p.board.shape == (tile.H, tile.W) and p.stats["depth"] == wc.RANK_HALO, (p.rank, p.stats)
            if "schedule" in kw:
                assert p.stats["schedule"] == kw["schedule"], (p.rank, p.stats)
            bands = check_plan(gol, p.stats, tile, wc.RANK_KDEPTH, boundary, census, region=region)
        got = wc.check_ranks(H, W, parts, ref, bands)
        cpu = wc.run_ranks(gol, P, H, W, "cpu", script, rule=rule, boundary=boundary, census=census, **kw)
        assert [(p.row0, p.col0) for p in cpu] == [(p.row0, p.col0) for p in parts]
        assert np.array_equal(wc.assemble(H, W, cpu), got)
        if census:
            assert len(set(counts.tolist())) >= 2
            for p in parts + cpu:
                start, series, pop = p.result
                assert start == 0 and series.dtype == np.uint64 and np.array_equal(series, counts), (p.rank, series.tolist())
                assert pop == int(counts[-1]), (p.rank, pop)


# ----- 6. the 1-rank RCCL communicator -----

@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


def test_rccl_self(gol, rccl):
    """A bounded census on 96 x 4096, the rank its own y neighbour through the transport: ghost rows stored by the
    exchanges and by the earlier pass, all of them beyond the board."""
    s, K, R, gens = wc.Shape(96, 4096, 1, 2, 64), 8, 16, wc.RANK_GENS
    counts, boards = wc.history(s.H, s.W, B1, "dead", gens)
    sim = gol.Simulation(s.H, rccl, backend="hip", device=0, self_exchange=True, width=s.W, rule=B1, boundary="dead",
                         halo_depth=R, kernel_depth=K, subtiles=0, census=True)
    sim.init(5, seed=wc.SEED)
    bands = check_plan(gol, sim.stats(), s, K, "dead", True, region=(-8, s.H + 8, 0, 64))
    sim.step(gens)
    st = sim.stats()
    assert st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
    wc.check_census(sim, counts, boards[gens], K, bands)
    sim.synchronize()


# ----- 7. views on the wide board -----

def test_views(gol):
    """k_density with more than one 64-lane word group and blocks that span two groups; a window across the seam
    between segments 0 and 1."""
    s, K, gens = wc.Shape(64, 8000, 2, 1, 64), 8, 9
    sim = _sim(gol, s, K, HIGHLIFE, "dead")
    check_plan(gol, sim.stats(), s, K, "dead")
    sim.step(gens)
    ref = wc.board_after(s, HIGHLIFE, "dead", gens, gens)
    assert not np.array_equal(ref, wc.board_after(s, HIGHLIFE, "torus", gens, gens))
    for br, bc in [(7, 64 * 3), (64, 64 * 125), (1, 64)]:
        d = sim.density(br, bc)
        want = np_density(ref, br, bc)
        assert d.dtype == np.uint32 and d.shape == want.shape and np.array_equal(d, want), (br, bc, int((d != want).sum()))
    assert np.array_equal(sim.window(10, 3960, 20, 80), ref[10:30, 3960:4040])
    assert np.array_equal(sim.window(0, 0, s.H, s.W), ref)
    assert sim.population() == int(ref.sum())
