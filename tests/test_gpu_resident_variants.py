"""step_resident<NW, B> (csrc/src/hip/resident_kernel.hip) in all 14 variants the planner can pick -- 16 waves x
{2, 3, 4, 5, 6, 8} rows and 8 waves x {3, 4, 5, 6, 8, 10, 12, 16} rows -- bit for bit against numpy (B3/S23 on the
torus), on the boards of resident_cases.py; test_resident_plans.py asserts on the CPU that those boards contain what is
claimed here.

Every run is pinned: kernel="resident", kernel_depth = kin, subtiles = 0, GOL_SPINUP_MS=0 and the test knob
GOL_RESIDENT=tiles,nw, which makes the planner cut a small board as for a card of ``tiles`` CUs with ``nw`` waves per
tile (it can only plan fewer tiles than the card has CUs).  Before a board is compared the test asserts the whole
``resident@kin(<tiles> tiles x <nw> waves x <B> rows)`` string of stats()["kernel"] against resident_cases' prediction;
then the board against numpy_step and population() against the numpy sum.  A wrong board fails with
wide_cases.mismatch_report.  A run of G generations is one launch of an odd number S of supersteps.

  * band range ends:   per variant a tile of T = NW x B extended rows exactly, and one at the smallest T that plans this
                       B (whole waves empty), G = kin and 3 kin;
  * superstep cuts:    16 x 4 and 8 x 8 at the four depths, G in {1, 2, kin - 1, kin, kin + 1, 2 kin, 2 kin + 1,
                       3 kin + 1}: S = 1, S bumped to odd (kmax < kin: a smaller T than planned), two lengths;
  * tile shapes:       one-row tiles (the halo spans kin tiles each way), tiles shorter than kin, tiles of >= 2 kin rows,
                       two heights in a plan, for every variant that can have them; one tile alone on 64 rows at kin = 24
                       (T > H: its halo is its own rows); two tiles side by side; 2 x 2 tiles;
  * widths:            64 and 128 columns (many segments packed in a tile), 3968, 4032, 4096 (full tiles and a packed
                       one), 7936 (the seam), at one variant per NW;
  * launch sequences:  one simulation stepped (kin, 1, 2 kin + 1, kin - 1, 3 kin), eagerly and with run_hint = 2 kin + 1
                       (graph replays), the board compared after every step: counters carried over launches, the result
                       buffer's parity;
  * two tiles per CU:  the boards resident_cases.two_per_cu_case finds.

The 256-CU plan is test_gpu_resident.py's (the 8192^2 board); no wait is made to time out here."""
import numpy as np
import pytest

import resident_cases as rc
import wide_cases as wc
from resident_cases import VARIANTS, case_id, vid

pytestmark = pytest.mark.gpu


def start(gol, monkeypatch, c, **kw):
    """A pinned simulation of case ``c``; the kernel string is asserted here."""
    monkeypatch.setenv("GOL_RESIDENT", f"{c.tiles},{c.nw}")
    monkeypatch.setenv("GOL_SPINUP_MS", "0")
    sim = gol.Simulation(c.H, backend="hip", device=0, width=c.W, kernel="resident", kernel_depth=c.kin, subtiles=0,
                         **kw).init(5, seed=wc.SEED)
    p = rc.plan(c.H, c.W, c.kin, c.tiles, c.nw)
    st = sim.stats()
    assert st["kernel"] == rc.kernel_name(c.kin, p, c.nw), (st["kernel"], c)
    assert st["plan_waves"] == p.tiles, st
    return sim, wc.bands_of(p.waves)


def check(sim, c, bands, gens):
    ref = rc.board_after(c.H, c.W, gens)
    wc.check_board(sim.board(), ref, c.kin, bands)
    assert sim.population() == int(ref.sum(dtype=np.int64))


def run(gol, monkeypatch, c, gens):
    sim, bands = start(gol, monkeypatch, c)
    sim.step(gens)
    check(sim, c, bands, gens)


@pytest.mark.parametrize("end", ["fill", "least"])
@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_band_range_ends(gol, monkeypatch, v, end):
    """T = NW x B exactly (the top wave's last register row is the last extended row) and the smallest T that plans
    this B (whole waves only keep the barrier); one superstep and three, kmax = kin."""
    c = rc.fill_case(*v) if end == "fill" else rc.least_case(*v)
    assert (c.nw, c.B) == v
    for gens in (c.kin, 3 * c.kin):
        run(gol, monkeypatch, c, gens)


@pytest.mark.parametrize("kin", rc.DEPTHS)
@pytest.mark.parametrize("v", rc.CUT_VARIANTS, ids=vid)
def test_superstep_cuts(gol, monkeypatch, v, kin):
    c = rc.cut_case(v[0], kin)
    assert (c.nw, c.B) == v
    for gens in rc.cut_gens(kin):
        run(gol, monkeypatch, c, gens)


@pytest.mark.parametrize("name,c", rc.shape_cases(), ids=lambda x: x if isinstance(x, str) else case_id(x))
def test_tile_shapes(gol, monkeypatch, name, c):
    run(gol, monkeypatch, c, 3 * c.kin)


@pytest.mark.parametrize("W", rc.WIDTHS)
@pytest.mark.parametrize("nw", rc.WAVES)
def test_widths(gol, monkeypatch, nw, W):
    c = rc.width_case(W, nw)
    run(gol, monkeypatch, c, 3 * c.kin)


@pytest.mark.parametrize("hinted", [False, True], ids=["eager", "hinted"])
@pytest.mark.parametrize("c", rc.seq_cases(), ids=case_id)
def test_launch_sequences(gol, monkeypatch, c, hinted):
    """Five launches of one simulation, 1, 1, 3, 1 and 3 supersteps: the per-tile counters carry over, the result
    lands in the other buffer each time.  Hinted, runs of 2 kin + 1 generations replay a captured graph (the third
    step, and the first 2 kin + 1 generations of the fifth)."""
    sim, bands = start(gol, monkeypatch, c, **({"run_hint": 2 * c.kin + 1} if hinted else {}))
    total = 0
    for gens in rc.seq_gens(c.kin):
        sim.step(gens)
        total += gens
        check(sim, c, bands, total)
    assert sim.stats()["graph_launches"] >= (2 if hinted else 0), sim.stats()


@pytest.mark.parametrize("nw", rc.WAVES)
def test_two_tiles_per_cu(gol, monkeypatch, nw):
    """The planner's second round: one-row segments of an 81 x 64 board packed into four tiles of 64 / nw-row bands."""
    c = rc.two_per_cu_case(nw)
    assert c is not None and rc.plan(c.H, c.W, c.kin, c.tiles, c.nw).per_cu == 2
    for gens in (c.kin, 3 * c.kin):
        run(gol, monkeypatch, c, gens)


def test_knob_is_checked(gol, monkeypatch):
    for bad in ["4", "4,12", "0,16", "4,16,1", "x"]:
        monkeypatch.setenv("GOL_RESIDENT", bad)
        with pytest.raises(Exception, match="GOL_RESIDENT"):
            gol.Simulation(64, backend="hip", device=0, kernel="resident", kernel_depth=8, subtiles=0).init(5, seed=1)
