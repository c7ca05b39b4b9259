"""The case lists of resident_cases.py really contain what test_gpu_resident_variants.py relies on: every variant of
step_resident the planner can pick, on boards whose tiles fill NW x B exactly or leave whole waves empty, are one row
or many rows tall, come in two heights, reload their own rows, or are packed from many narrow segments.  The mirror
of ``res_plan`` / ``res_launch`` is held against the source text and against values worked out by hand; the tiles come
from ``build_plan`` through the bindings, padding tiles dropped.  No GPU is needed."""
import os
import re

import numpy as np
import pytest

import resident_cases as rc
import wide_cases as wc
from resident_cases import VARIANTS, case_id, vid

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(REPO, "csrc", "src", "hip", "resident_kernel.hip")
ENGINE = os.path.join(REPO, "csrc", "src", "engine", "engine_hip_resident.hip")


@pytest.fixture(scope="module")
def kernel_src():
    with open(KERNEL) as f:
        return f.read()


@pytest.fixture(scope="module")
def engine_src():
    with open(ENGINE) as f:
        return f.read()


def plan_of(c):
    p = rc.plan(c.H, c.W, c.kin, c.tiles, c.nw)
    assert p is not None and p.B == c.B, (c, p)
    return p


# ----- the table -----

def test_reachable_variants(kernel_src):
    """The planner's arithmetic reaches these fourteen and the kernel dispatches exactly them."""
    assert list(VARIANTS) == [(16, 2), (16, 3), (16, 4), (16, 5), (16, 6), (16, 8),
                              (8, 3), (8, 4), (8, 5), (8, 6), (8, 8), (8, 10), (8, 12), (8, 16)]
    table = re.findall(r"case (\d+): return \(const void\*\)step_resident<(\d+), (\d+)>;", kernel_src)
    assert all(a == b for a, _, b in table)
    assert sorted((int(nw), int(b)) for _, nw, b in table) == sorted(VARIANTS)
    assert len(re.findall(r"step_resident<\d+, \d+>", kernel_src)) == len(VARIANTS)  # nothing instantiated beside them
    m = re.search(r"for \(int b : \{([\d, ]+)\}\)", kernel_src)
    assert [int(x) for x in m.group(1).split(",")] == rc.BANDS
    assert "WRAPY" not in kernel_src and "B == 1" not in kernel_src


def test_mirror_matches_the_source(kernel_src, engine_src):
    for line in [
        "const int bmax = (per_cu == 1 ? 128 : 64) / nw;",
        "const i64 rows = balanced_rows_per_chunk(rg, L_.nw, L_.h, kin, (i64)per_cu * cus, 1, true);",
        "if (rows + 2 * (i64)kin > nw * (i64)bmax) continue;",
        "const int B = hipk::resident_band_rows((int)ceil_div(rows + 2 * (i64)kin, nw));",
        "if (B <= 0 || B > bmax) continue;",
        "if (live > (i64)per_cu * cus) continue;",
        "if (tallest + 2 * (i64)kin > nw * (i64)B) continue;",
        "cus = std::min<i64>(t, cus_);",
        "int S = (G + rp.kin - 1) / rp.kin;",
        "S += (S % 2 == 0);",
        "p.kmax = (G + S - 1) / S;",
    ]:
        assert line in engine_src, line
    for line in [
        "const int ks = rp.G / rp.S + (s <= rp.G % rp.S ? 1 : 0);",
        "const bool active = b0 + B > g - 1 && b0 < T - g + 1;",
        "const int T = nrows + 2 * K;",
        "const int K = rp.kmax;",
        "const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);",
    ]:
        assert line in kernel_src, line


def test_cut_by_hand():
    assert rc.cut(1, 8) == (1, 1, (1,)) and rc.cut(8, 8) == (1, 8, (8,))     # S = 1: no exchange in the kernel
    assert rc.cut(9, 8) == (3, 3, (3, 3, 3))                                  # 2 supersteps made 3: kmax < kin
    assert rc.cut(16, 8) == (3, 6, (6, 5, 5))                                 # ... and of two lengths
    assert rc.cut(17, 8) == (3, 6, (6, 6, 5))
    assert rc.cut(25, 8) == (5, 5, (5, 5, 5, 5, 5)) and rc.cut(73, 24) == (5, 15, (15, 15, 15, 14, 14))
    assert rc.cut(72, 24) == (3, 24, (24, 24, 24))
    for kin in rc.DEPTHS:
        cuts = [rc.cut(G, kin) for G in rc.cut_gens(kin)]
        assert all(c.S % 2 == 1 and sum(c.ks) == G and max(c.ks) == c.kmax <= kin
                   for c, G in zip(cuts, rc.cut_gens(kin)))
        assert [c.S for c in cuts] == [1, 1, 1, 1, 3, 3, 3, 5]
        assert any(c.kmax < kin and c.S > 1 for c in cuts) and any(len(set(c.ks)) == 2 for c in cuts)


def test_trapezoid_by_hand():
    # 16 waves x 4 rows, T = 49 (rows 0 .. 48): wave 12 holds row 48, waves 13 .. 15 nothing
    assert rc.empty_waves(16, 4, 49) == [13, 14, 15]
    assert rc.inactive(16, 4, 1, 49) == [13, 14, 15]          # generation 1 reads rows [0, 49)
    assert rc.inactive(16, 4, 2, 49) == [12, 13, 14, 15]      # generation 2 reads rows [1, 48)
    assert rc.inactive(16, 4, 6, 49) == [0, 11, 12, 13, 14, 15]  # rows [5, 44): band 0 (rows 0 .. 3) is out
    assert rc.inactive(16, 4, 24, 49) == [0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15]  # rows [23, 26)
    assert rc.inactive(8, 16, 1, 128) == [] and rc.empty_waves(8, 16, 128) == []


# ----- the boards -----

def check_tiles(gol, c):
    """The plan the engine would upload: every lane of a tile has the tile's nrows (the kernel takes it from one
    lane), the tiles cover the board once, and the padding is to whole blocks of four."""
    p = plan_of(c)
    lanes, st = gol.native.build_plan([(0, c.H, 0, c.W // 64)], c.W // 64, c.H, p.rows, c.kin, True, False)
    lanes = np.asarray(lanes).reshape(-1, 64, 4)
    assert (lanes[:, :, 3] == lanes[:, :1, 3]).all()
    assert p.tiles == st["waves"] == lanes.shape[0] and p.tiles % 4 == 0 and p.tiles - p.live < 4
    assert p.live == int((lanes[:, 0, 3] > 0).sum()) <= p.per_cu * min(c.tiles, rc.CUS)
    assert wc.covers_once(p.waves, (0, c.H, 0, c.W // 64))
    assert p.T == max(p.heights) + 2 * c.kin <= c.nw * c.B <= rc.CAP[p.per_cu]
    assert p.T > c.nw * rc.prev_band(c.B)
    return p


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_band_range_ends(gol, v):
    nw, B = v
    f, l = rc.fill_case(nw, B), rc.least_case(nw, B)
    pf, pl = check_tiles(gol, f), check_tiles(gol, l)
    assert (f.nw, f.B) == v == (l.nw, l.B)
    assert pf.T == nw * B and rc.empty_waves(nw, B, pf.T) == [] and rc.inactive(nw, B, 1, pf.T) == []
    assert pl.T == max(nw * rc.prev_band(B) + 1, 17)
    empty = rc.empty_waves(nw, B, pl.T)
    assert empty and empty[-1] == nw - 1 and rc.inactive(nw, B, 1, pl.T) == empty
    for c, p in ((f, pf), (l, pl)):
        assert len(p.heights) == 1 and c.W == rc.FULL_W and c.H * c.W <= 1 << 20
        for G in (c.kin, 3 * c.kin):
            assert rc.cut(G, c.kin).kmax == c.kin  # the planned T is the kernel's
        # the last generation of a superstep reads rows [kin - 1, T - kin + 1): the bands wholly outside skip it
        last = rc.inactive(nw, B, c.kin, p.T)
        rows = set(range(c.kin - 1, p.T - c.kin + 1))
        assert last == [w for w in range(nw) if not rows & set(range(w * B, (w + 1) * B))]
        assert set(last) >= set(rc.inactive(nw, B, 1, p.T))


def test_shape_cases(gol):
    cases = rc.shape_cases()
    by = {}
    for name, c in cases:
        by.setdefault(name, []).append(c)
        p = check_tiles(gol, c)
        reach = rc.halo_reach(p, c.H, c.kin)
        if name == "one_row":
            assert p.heights == (1,) and reach == c.kin and p.live == 64
        elif name == "short":
            assert len(p.heights) == 1 and 1 < p.heights[0] < c.kin and reach >= 2
        elif name == "tall":
            assert p.heights[0] >= 2 * c.kin and reach == 1
        elif name == "two_heights":
            assert len(p.heights) == 2 and p.heights[0] == p.heights[1] + 1
        elif name == "alone":
            assert p.live == 1 and p.T == 112 > c.H == 64 and c.kin == 24 and (c.nw, c.B) in ((16, 8), (8, 16))
        elif name == "pair":
            assert p.live == 2 and p.heights == (64,) and all(wc.is_full_width(w) for w in p.waves)
            assert p.T > c.H  # each also reloads rows it published itself
        elif name == "ring4":
            assert p.live == 4 and wc.bands_of(p.waves) == [(0, 32), (32, 32)] and c.kin < 32
    variants = lambda name: {(c.nw, c.B) for c in by[name]}
    # a one-row tile has T = 2 kin + 1 in {17, 25, 33, 49}; a tile shorter than kin has T < 72; more own rows than
    # halo rows is every band height
    assert variants("one_row") == {(16, 2), (16, 3), (16, 4), (8, 3), (8, 4), (8, 5), (8, 8)}
    assert variants("short") == {v for v in VARIANTS if v[0] * rc.prev_band(v[1]) + 1 < 72}
    assert variants("tall") == set(VARIANTS) - {(8, 3)}  # (8 x 3: T <= 24 < 16 + 2 x 8 + ...: nrows <= 8)
    assert variants("two_heights") == set(VARIANTS)
    assert len(by["alone"]) == len(by["pair"]) == len(by["ring4"]) == 2
    assert all(c.H * c.W <= 1 << 20 for _, c in cases)


def test_cut_cases(gol):
    assert rc.CUT_VARIANTS == [(16, 4), (8, 8)] and set(rc.CUT_VARIANTS) <= set(VARIANTS)
    for nw, B in rc.CUT_VARIANTS:
        for kin in rc.DEPTHS:
            c = rc.cut_case(nw, kin)
            p = check_tiles(gol, c)
            assert (c.nw, c.B, c.kin) == (nw, B, kin) and p.live == 4 and len(p.heights) == 1
            # a cut with kmax < kin runs on a smaller T than planned: more waves are empty
            k3 = rc.cut(kin + 1, kin).kmax
            assert k3 < kin
            assert len(rc.empty_waves(nw, B, p.heights[0] + 2 * k3)) > len(rc.empty_waves(nw, B, p.T))


def test_width_cases(gol):
    assert set(rc.WIDTH_VARIANTS) <= set(VARIANTS)
    for nw, B in rc.WIDTH_VARIANTS:
        got = {}
        for W in rc.WIDTHS:
            c = rc.width_case(W, nw)
            p = check_tiles(gol, c)
            got[W] = p
            assert c.nw == nw and (c.B == B or W < rc.FULL_W) and c.H * c.W <= 1 << 20
        segs = lambda W: sorted({n for w in got[W].waves for _, _, n in wc.segments(w)})
        for W in (64, 128):  # many short segments to a tile
            assert segs(W) == [W // 64] and all(wc.is_packed(w) for w in got[W].waves)
            assert min(len(wc.segments(w)) for w in got[W].waves[:-1]) >= 64 // (W // 64 + 2)
        assert all(int(w.col[0]) == 0 and int(w.col[2]) == 0 for w in got[64].waves)  # the word is its own neighbour
        assert segs(3968) == [62] and all(wc.is_full_width(w) for w in got[3968].waves)
        assert segs(4032) == [1, 62] and segs(4096) == [2, 62] and segs(7936) == [62]
        for W in (4032, 4096):  # full tiles and one packed tile of the bands' remainders
            packed = [w for w in got[W].waves if not wc.is_full_width(w)]
            assert len(packed) == 1 and len(wc.segments(packed[0])) == len(wc.bands_of(got[W].waves)) >= 2
        assert sorted({c for w in got[7936].waves for _, c, _ in wc.segments(w)}) == [0, 62]  # the seam


def test_launch_sequences(gol):
    cases = rc.seq_cases()
    assert sorted(c.nw for c in cases) == [8, 16]
    for c in cases:
        check_tiles(gol, c)
        gens = rc.seq_gens(c.kin)
        assert gens == [c.kin, 1, 2 * c.kin + 1, c.kin - 1, 3 * c.kin]
        S = [rc.cut(g, c.kin).S for g in gens]
        assert S == [1, 1, 3, 1, 3]  # counters move by S - 1 per launch: 0, 0, 2, 0, 2
        assert 2 * c.kin + 1 < 64 <= 3 * c.kin + 64  # the hinted length is below the resident run depth's floor


def test_two_per_cu(gol):
    """The planner's second round (two tiles per CU, tiles of at most 64 extended rows) is reachable under the knob,
    because a plan is counted in blocks of four waves: ``tiles`` = 2 makes the first round the whole board."""
    for nw in rc.WAVES:
        c = rc.two_per_cu_case(nw)
        assert c == rc.Case(81, 64, 24, 2, nw, 64 // nw)
        p = check_tiles(gol, c)
        assert p.per_cu == 2 and p.live == 4 and p.heights == (1,) and p.T == 49 and all(wc.is_packed(w) for w in p.waves)
        # the first round is refused: one band of 81 rows, 129 extended rows
        assert gol.native.balanced_rows_per_chunk([(0, 81, 0, 1)], 1, 81, 24, 2, 1, True) == 81
        assert rc.plan(80, 64, 24, 2, nw).per_cu == 1


def test_every_variant_has_gpu_cases():
    seen = {(c.nw, c.B) for v in VARIANTS for c in (rc.fill_case(*v), rc.least_case(*v))}
    assert seen == set(VARIANTS)
    ids = [case_id(c) for _, c in rc.shape_cases()]
    assert len(ids) == len(set(zip(ids, [n for n, _ in rc.shape_cases()])))
