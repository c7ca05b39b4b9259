"""step_tile and step_tile_fold (csrc/src/hip/tile_device.hpp), the LDS tile kernels, in all 72 instantiations --
NW in {4, 8, 16} waves x LV in {1, 2, 4} generations per LDS pass x double-buffered / in place x plain / folded x
WRAPY on / off -- bit for bit against numpy (B3/S23 on the torus), on the boards of tile_cases.py; test_tile_plans.py
asserts on the CPU that those boards contain what is claimed here.

Every test names its variant (tile_waves, GOL_TILE_LEVELS, GOL_TILE_INPLACE, GOL_TILE_FOLD, read when the engine is
built) and asserts from stats() that it ran: the kernel, the pass cut and the whole ``tile_plan=`` entry -- layout,
rows per tile, tiles and levels -- so a forced fold that the planner drops fails instead of passing as a plain tile.
Unless it says otherwise a test runs 2K + 1 generations at kernel_depth = halo_depth = K: two full passes and a
one-generation remainder superstep.  A wrong board fails with tile_cases.tile_report.

Which test launches which instantiation (kernel<NW, WRAPY, LV, in place>), asserting the variant from stats():

    step_tile<NW, true, LV, IP>, step_tile_fold<NW, true, LV, IP>, all 36:        test_variant_sweep
    step_tile<NW, false, LV, IP>, step_tile_fold<NW, false, LV, IP>, all 36:      test_thread_ranks_every_variant
    the 18 at NW = 8, WRAPY true again on interior / band regions:                test_split_schedule
    step_tile<8, false, 4, false>, step_tile_fold<8, false, 4, false> again:      test_thread_ranks

WRAPY follows from the rank: one rank is its own N / S neighbour and streams rows modulo h, also in the split
schedule; two thread ranks stream ghost rows, and their first pass stores the ghost rows the second reads.  Through the
engine the deepest pass is 32 generations (HipEngine caps kernel "tile" there; launch_step_tile itself takes 64), so
the depth sweep's K = 48 and 64 run supersteps of one and of two passes of 32, which is asserted.  At 32 generations
every variant still holds 64 rows or more, so the engine's "leaves no LDS rows" refusal cannot be provoked; the
capacity mirrors are checked through the rows the engine reports for plain tiles clamped to the capacity and through
its refusal of a folded tile one row above it.  The ``tiles`` of an entry count the plan's workgroups, which
``build_plan`` pads to a multiple of 4."""
import numpy as np
import pytest

import tile_cases as tc
import wide_cases as wc
from gol_amd.ops import numpy_step
from tile_cases import VARIANTS, Variant, vid

pytestmark = pytest.mark.gpu

BIG = 1 << 20  # rows_per_wave: as tall as the LDS allows


@pytest.fixture(autouse=True)
def _no_spinup(monkeypatch):
    monkeypatch.setenv("GOL_SPINUP_MS", "0")


def set_variant(monkeypatch, v):
    monkeypatch.setenv("GOL_TILE_LEVELS", str(v.lv))
    monkeypatch.setenv("GOL_TILE_INPLACE", "1" if v.inplace else "0")
    monkeypatch.setenv("GOL_TILE_FOLD", "1" if v.fold else "0")


def make(gol, monkeypatch, v, H, W, K, rows, R=None, **kw):
    set_variant(monkeypatch, v)
    return gol.Simulation(H, backend="hip", device=0, width=W, kernel="tile", kernel_depth=K,
                          halo_depth=K if R is None else R, tile_waves=v.nw, rows_per_wave=rows, subtiles=0,
                          **kw).init(5, seed=tc.SEED)


def reported_rows(v, rows, K):
    """Rows per tile of the plan: a plain tile is clamped to the LDS capacity, a folded one must fit as asked."""
    return rows if v.fold else min(rows, tc.max_rows(v, K))


def check_ran(gol, st, v, H, W, K, rows, R=None, regions=None, name="tile_plan", kernel="tile", schedule="local",
              fold=None):
    """The tile kernel at depth K on the plan ``build_plan`` gives for the same arguments, as variant ``v``; returns
    the plan's tiles ``[(row0, nrows)]``."""
    R = K if R is None else R
    S, depths = tc.engine_cut(K) if R == K else (R, [K] * (R // K))
    fold = v.fold if fold is None else fold
    assert st["kernel"] == kernel and st["schedule"] == schedule and st["tile_waves"] == v.nw, st
    assert st["depth"] == R and st["kernel_depth"] == min(K, tc.ENGINE_MAX_DEPTH), st
    tuning = st["tuning"].split()
    assert tc.tile_cut(S, depths) in tuning, st["tuning"]
    kp = min(K, tc.ENGINE_MAX_DEPTH)
    nw = wc.nwords(W)
    vv = v._replace(fold=fold)
    rr = reported_rows(vv, rows, kp)
    waves, pst = tc.plan_tiles(gol, regions or [(0, H, 0, nw)], W, H, rr, kp, fold)
    want = tc.entry(name, vv, rr, pst["waves"])  # (the plan's workgroups: build_plan pads them to a multiple of 4)
    assert want in tuning, (want, st["tuning"])
    return sorted({(int(w.row0[l]), w.nrows) for w in waves for l in range(64) if w.store[l]})


def run_case(gol, monkeypatch, v, H, W, K, rows, total=None):
    sim = make(gol, monkeypatch, v, H, W, K, rows)
    tiles = check_ran(gol, sim.stats(), v, H, W, K, rows)
    gens = tc.gens_of(K)
    sim.step(gens)
    ref = wc.history(H, W, wc.CONWAY, "torus", total or gens)[1][gens]
    tc.check_board(sim.board(), ref, K, tiles, v.fold, tc.FOLD_SEG if v.fold else wc.SEG)
    return tiles


# ----- 1. every variant with WRAPY, on the boards that reach every feature of its band arithmetic -----

@pytest.mark.parametrize("width", ["192", "full"])
@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_variant_sweep(gol, monkeypatch, v, width):
    """tile_cases.sweep_cases(v): every n mod 6 (mod 3) of the band stream, a one-row band at 2 levels, idle waves, a
    short last band, bands thinner than LV, every remainder pass, both swap parities; folded: T odd and even, the
    mirror rows written by two waves, tiles of 14, 15, 27 and 28 rows.  At 192 columns (3-word segments) and at the
    family's full-width shape: 1920 columns folded (one 32-lane segment), 3968 plain (one 64-lane segment)."""
    W = tc.COLS if width == "192" else (tc.FULL_FOLD[0] if v.fold else wc.S3968.W)
    for c in tc.sweep_cases(v):
        tiles = run_case(gol, monkeypatch, v, c.H, W, c.K, c.rows)
        assert tiles == tc.tiles_of(c.H, c.rows), (c, tiles)


# ----- 2. depths -----

@pytest.mark.parametrize("v", [tc.DEFAULT, tc.DEFAULT_FOLD], ids=vid)
@pytest.mark.parametrize("K", tc.DEPTH_SWEEP)
def test_depth_sweep(gol, monkeypatch, v, K):
    """The tallest tile the depth allows (the reported rows are the capacity mirror's) and the shortest: one row, or
    for folded tiles the shortest bands of rows_per_wave = 28."""
    kp = min(K, tc.ENGINE_MAX_DEPTH)
    cap = tc.max_rows(v, kp)
    assert cap >= K
    tiles = run_case(gol, monkeypatch, v, cap, tc.COLS, K, cap if v.fold else BIG)
    assert tiles == [(0, cap)]
    if v.fold:
        H = max(tc.FOLD_MIN_ROWS + 1, K + (K + 1) % 2)  # two or three tiles, not all of one height
        tiles = run_case(gol, monkeypatch, v, H, tc.COLS, K, tc.FOLD_MIN_ROWS)
        assert len(tiles) >= 2 and all(tc.FOLD_MIN_ROWS // 2 <= n <= tc.FOLD_MIN_ROWS for _, n in tiles), tiles
    else:
        tiles = run_case(gol, monkeypatch, v, max(K, 3), tc.COLS, K, 1)
        assert tiles == [(r, 1) for r in range(max(K, 3))]


@pytest.mark.parametrize("v", [Variant(nw, 4, ip, True) for nw in tc.CAPACITY_WAVES for ip in (False, True)], ids=vid)
@pytest.mark.parametrize("K", tc.CAPACITY_DEPTHS)
def test_fold_refused_above_capacity(gol, monkeypatch, v, K):
    """A folded tile one row above the capacity mirror: the engine's refusal names the capacity."""
    cap = tc.max_rows(v, K)
    with pytest.raises(Exception, match=rf"GOL_TILE_FOLD: {cap + 1} rows per folded tile outside 28\.\.{cap} at depth {K}"):
        make(gol, monkeypatch, v, 2 * (cap + 1), tc.COLS, K, cap + 1)


# ----- 3. tiles at the LDS capacity -----

@pytest.mark.parametrize("K", tc.CAPACITY_DEPTHS)
@pytest.mark.parametrize("v", [Variant(nw, 4, ip, fold) for fold in (False, True) for ip in (False, True)
                               for nw in tc.CAPACITY_WAVES], ids=vid)
def test_at_capacity(gol, monkeypatch, v, K):
    """Two tiles of exactly tile_max_rows rows (the tuner runs tiles at the capacity); folded also one row below it:
    both parities of T."""
    cap = tc.max_rows(v, K)
    assert tc.lds_rows(v, cap, K) <= tc.LDS_ROWS and cap >= tc.FOLD_MIN_ROWS
    tiles = run_case(gol, monkeypatch, v, 2 * cap, tc.COLS, K, cap if v.fold else BIG)
    assert tiles == [(0, cap), (cap, cap)]
    if v.fold:
        tiles = run_case(gol, monkeypatch, v, 2 * cap - 2, tc.COLS, K, cap - 1)
        assert tiles == [(0, cap - 1), (cap - 1, cap - 1)]
        assert tc.fold_geometry(cap, K).odd and not tc.fold_geometry(cap - 1, K).odd


# ----- 4. wide boards: full-width segments, the tail word, packed remainders, a seam -----

@pytest.mark.parametrize("lv", tc.LEVELS)
@pytest.mark.parametrize("inplace", [False, True], ids=["double", "inplace"])
@pytest.mark.parametrize("s", tc.WIDE, ids=wc.shape_id)
def test_wide_plain(gol, monkeypatch, s, inplace, lv):
    rows = (s.H + 1) // 2
    for K in tc.WIDE_DEPTHS:
        tiles = run_case(gol, monkeypatch, Variant(8, lv, inplace, False), s.H, s.W, K, rows, tc.gens_of(max(tc.WIDE_DEPTHS)))
        assert tiles == tc.tiles_of(s.H, rows)


@pytest.mark.parametrize("lv", tc.LEVELS)
@pytest.mark.parametrize("inplace", [False, True], ids=["fold", "fold-inplace"])
@pytest.mark.parametrize("W", tc.FULL_FOLD)
def test_wide_fold(gol, monkeypatch, W, inplace, lv):
    """Tiles of 30 and 29 rows: 1920 columns are one full 32-lane folded segment, 2048 add a packed 2-word one."""
    H, rows = 59, 30
    for K in tc.WIDE_DEPTHS:
        tiles = run_case(gol, monkeypatch, Variant(8, lv, inplace, True), H, W, K, rows, tc.gens_of(max(tc.WIDE_DEPTHS)))
        assert tiles == [(0, 30), (30, 29)]


# ----- 5. the split schedule: interior and band regions (one rank: WRAPY) -----

@pytest.mark.parametrize("v", [x for x in VARIANTS if x.nw == 8], ids=vid)
@pytest.mark.parametrize("K", tc.SPLIT_DEPTHS)
@pytest.mark.parametrize("H,W", tc.SPLIT_BOARDS)
def test_split_schedule(gol, monkeypatch, H, W, K, v):
    """force_split: the interior (rows K .. H - K) on one stream, the two bands of K rows on the other.  The interior
    folds when asked; the bands never do (a folded plan needs a region of 28 rows), each is one plain tile."""
    sim = make(gol, monkeypatch, v, H, W, K, tc.SPLIT_ROWS, force_split=True)
    st = sim.stats()
    nw = wc.nwords(W)
    interior, bands = tc.split_regions(H, nw, K)
    t1 = check_ran(gol, st, v, H, W, K, tc.SPLIT_ROWS, regions=interior, name="tile_plan1",
                   kernel="tile+boundary:tile", schedule="split")
    t2 = check_ran(gol, st, v, H, W, K, tc.SPLIT_ROWS, regions=bands, name="tile_plan2",
                   kernel="tile+boundary:tile", schedule="split", fold=False)
    assert t2 == [(0, K), (H - K, K)] and "tile_plan=" not in st["tuning"]
    gens = tc.gens_of(K)
    sim.step(gens)
    ref = wc.history(H, W, wc.CONWAY, "torus", tc.gens_of(max(tc.SPLIT_DEPTHS)))[1][gens]
    tc.check_board(sim.board(), ref, K, sorted(t1 + t2), v.fold, tc.FOLD_SEG if v.fold else wc.SEG)


# ----- 6. two thread ranks: ghost rows (WRAPY off) -----

def run_ranks(gol, monkeypatch, v, K):
    """96 x 4096 on two thread ranks sharing the GPU, supersteps of 2K generations in two passes of K: the first also
    stores the ghost rows the second reads.  4K + 3 generations: two supersteps and a remainder."""
    H, W = tc.RANKS_BOARD
    h, rows, gens = H // 2, 32, 4 * K + 3
    set_variant(monkeypatch, v)
    parts = wc.run_ranks(gol, 2, H, W, "hip", lambda s: s.step(gens), halo_depth=2 * K, kernel_depth=K, kernel="tile",
                         tile_waves=v.nw, rows_per_wave=rows, overlap=False, subtiles=0)
    for p in parts:
        assert p.board.shape == (h, W), p.board.shape
        tiles = check_ran(gol, p.stats, v, h, W, K, rows, R=2 * K, schedule="full")
        assert tiles == tc.tiles_of(h, rows)
    ref = wc.history(H, W, wc.CONWAY, "torus", gens)[1][gens]
    got = wc.assemble(H, W, parts)
    for p in parts:
        tc.check_board(p.board, ref[p.row0 : p.row0 + h], K, tiles, v.fold, tc.FOLD_SEG if v.fold else wc.SEG)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("v", [tc.DEFAULT, tc.DEFAULT_FOLD], ids=vid)
@pytest.mark.parametrize("K", tc.RANKS_DEPTHS)
def test_thread_ranks(gol, monkeypatch, K, v):
    run_ranks(gol, monkeypatch, v, K)


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_thread_ranks_every_variant(gol, monkeypatch, v):
    """K = 5: passes of 4 + 1, 2 + 2 + 1 and five of 1 level."""
    run_ranks(gol, monkeypatch, v, 5)


# ----- 7. the pair-shared rule at every row phase -----

@pytest.mark.parametrize("layout", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["double", "inplace", "fold", "fold-inplace"])
@pytest.mark.parametrize("K,lv", [(1, 1), (4, 4)])
def test_rule_phases(gol, monkeypatch, K, lv, layout):
    """A board with all 512 neighbourhoods centred on rows of every phase mod 3, in even and in odd columns: a wrong
    gate of the rule fails whatever the random density."""
    b = tc.phase_board()
    seen = tc.neighbourhoods_seen(b)
    assert all(seen[ph][par] == set(range(512)) for ph in range(3) for par in range(2))
    H, W = b.shape
    v = Variant(8, lv, layout[0], layout[1])
    rows = 46
    sim = make(gol, monkeypatch, v, H, W, K, rows)
    tiles = check_ran(gol, sim.stats(), v, H, W, K, rows)
    sim.set_board(b)
    done = 0
    for gens in (1, K, tc.gens_of(K)):
        sim.step(gens)
        done += gens
        tc.check_board(sim.board(), numpy_step(b, done), K, tiles, v.fold, tc.FOLD_SEG if v.fold else wc.SEG)


# ----- 8. word for word against step_temporal -----

@pytest.mark.parametrize("K", tc.CROSS_DEPTHS)
@pytest.mark.parametrize("H,W", tc.CROSS_BOARDS)
def test_against_temporal(gol, monkeypatch, H, W, K):
    """step_tile and step_tile_fold against step_temporal<K>, whose runner is separate."""
    gens = tc.gens_of(K)
    t = gol.Simulation(H, backend="hip", device=0, width=W, kernel="temporal", kernel_depth=K, halo_depth=K,
                       subtiles=0).init(5, seed=tc.SEED)
    assert t.stats()["kernel"] == "temporal" and t.stats()["kernel_depth"] == K, t.stats()
    t.step(gens)
    want = t.words()
    rows = tc.FOLD_MIN_ROWS
    for v in (tc.DEFAULT, tc.DEFAULT_FOLD):
        sim = make(gol, monkeypatch, v, H, W, K, rows)
        tiles = check_ran(gol, sim.stats(), v, H, W, K, rows)
        sim.step(gens)
        assert np.array_equal(sim.words(), want), tc.tile_report(
            sim.board(), t.board(), K, tiles, v.fold, tc.FOLD_SEG if v.fold else wc.SEG)
    ref = wc.history(H, W, wc.CONWAY, "torus", tc.gens_of(max(tc.CROSS_DEPTHS)))[1][gens]
    assert np.array_equal(t.board(), ref)
