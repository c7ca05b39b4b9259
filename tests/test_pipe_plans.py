"""The case lists of pipe_cases.py really contain what test_gpu_pipe_geometries.py relies on: for each of step_pipe's
24 geometries, boards whose bands between them take every branch of ``stage`` that any band can take, in each of its
three roles, and every path of the loader.  The mirror of the kernel's control flow is held against the source text
(constants, the fill length, the loop conditions, the geometry switch) and against values worked out by hand from the
source; the plans come from ``build_plan`` with the engine's arguments.  No GPU is needed."""
import os
import re

import pytest

import pipe_cases as pc
import wide_cases as wc
from pipe_cases import GEOMETRIES, gid

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "csrc", "src", "hip", "pipe_kernel.hip")


@pytest.fixture(scope="module")
def source():
    with open(SOURCE) as f:
        return f.read()


# ----- the mirror is not stale -----

def test_constants_match_the_source(source):
    got = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"constexpr int (kPipe\w+) = (\d+);", source))
    assert got == {"kPipeSync": pc.SYNC, "kPipeU": pc.QUEUE, "kPipeRing": pc.RING, "kPipeRing0": pc.RING0,
                   "kPipeLoadAhead": pc.LOAD_AHEAD}


def test_control_flow_matches_the_source(source):
    """The expressions the mirror copies, as the source writes them."""
    m = re.search(r"constexpr int i0 = (.+?);", source)
    assert m, "stage: no i0"
    expr = m.group(1)
    assert re.fullmatch(r"[\sL\d()+*/]+", expr), expr
    for L in pc.LEVELS:
        assert eval(expr.replace("/", "//"), {"L": L}) == pc.i0(L), (expr, L)  # (C++ integer division)
    for line in [
        "constexpr int U = RIN;",                                    # a loop turn is one ring: RING rows
        "if (n <= i0) {",                                            # short
        "in.ensure((u32)min(i0 + kPipeU, n));",                      # queue_partial below i0 + QUEUE
        "q[j] = i0 + j < n ? in.template read<i0 + j>() : make_uint2(0, 0);",
        "for (; i + U + kPipeU <= n; i += U) body(std::false_type{}, i);",
        "if (i + U < n) body(std::true_type{}, i + U);",             # tail2
        "if (TAIL && i + r >= n) return;",
        "constexpr int a = r - (S - 1) + kPipeU;",
        "if (!TAIL || nx + S <= n) {",                               # refill_full
        "} else if (nx < n) {",                                      # refill_partial
        "for (int j = 0; j < kPipeLoadAhead; ++j) issue(j);",
        "for (; i + kPipeLoadAhead < n; ++i) {",
        "if (j >= kPipeRing0) ctr_wait<true>(cons, freed, (u32)(j + 1 - kPipeRing0), acc_out);",
        "if (WRAPY && lrow < 0) lrow += p.h;",
        "const bool w = lrow == p.h;",
        "const int n = nrows + 2 * K - 2 * st * L;",
        "loader<WRAPY>(src, d, p, K, nrows + 2 * K, ring_of(0), ctr, ctr + NW);",
    ]:
        assert line in source, line
    assert re.search(r"if \(st == 0\)\s+run\(RingIn<kPipeRing0>\{\}\);\s+else\s+run\(RingIn<kPipeRing>\{\}\);", source)
    assert "if (wv == NW - 1) {" in source and "GlobalOut o;" in source and "RingOut o;" in source


def test_geometry_switch_matches_the_source(source):
    waves = re.findall(r"case (\d+): return pipe_kernel_nw<(\d+)>\(L, wrapy\);", source)
    levels = re.findall(r"case (\d+): return pipe_kernel_wrap<NW, (\d+)>\(wrapy\);", source)
    assert all(a == b for a, b in waves + levels)
    assert [int(a) for a, _ in waves] == pc.WAVES and [int(a) for a, _ in levels] == pc.LEVELS
    assert len(GEOMETRIES) == len(set(GEOMETRIES)) == 24
    assert sorted({pc.depth(*g) for g in GEOMETRIES})[0] == 4 and max(pc.depth(*g) for g in GEOMETRIES) == 60
    assert pc.GENS_TOTAL == 121


# ----- the mirror against values read off the source by hand -----

@pytest.mark.parametrize("L,n,want", [
    (1, 3, {"short"}),                                   # i0 = 3
    (4, 9, {"short"}),                                   # i0 = 9
    (3, 7, {"queue_partial", "steady0", "rem=1"}),       # i0 = 6: one row in the queue, no triple ends in the tail
    (4, 10, {"queue_partial", "steady0", "rem=1"}),
    (2, 8, {"queue_partial", "steady0", "rem=2"}),
    # i0 = 6, no steady turn (6 + 21 > 25); rows 6 .. 23 in the first tail pass, whose last triple finds one row left
    # to read (nx = 24); row 24 alone in the second
    (2, 6 + 19, {"steady0", "rem=19", "tail2", "refill_full", "refill_partial1"}),
    # i0 = 3, one steady turn to i = 21; rows 21 .. 23: the triple's refill finds nx = 24 = n
    (1, 3 + 21, {"steady1", "rem=3", "refill_none"}),
    # i0 = 6, turns to i = 24 and 42 (63 > 62); tail rows 42 .. 59, the last refill at nx = 60 reads two rows; 60, 61
    (3, 6 + 36 + 20, {"steady2plus", "rem=20", "tail2", "refill_full", "refill_partial2"}),
    # one steady turn needs i0 + 21 rows: one short of it
    (2, 6 + 20, {"steady0", "rem=20", "tail2", "refill_full", "refill_partial2"}),
    (2, 6 + 21, {"steady1", "rem=3", "refill_none"}),
])
def test_stage_mirror_by_hand(L, n, want):
    assert pc.stage_features(L, n) == want


def test_stage_rows_chain():
    """A stage emits n - 2L rows, which is what the next one streams; the last one emits the segment's rows."""
    for nw, L in GEOMETRIES:
        assert [pc.role_of(nw, st) for st in range(nw - 1)] == ["first"] + ["middle"] * (nw - 3) + ["last"]
        for nrows in (1, 7, 300):
            ns = [pc.stage_rows(nw, L, nrows, st) for st in range(nw - 1)]
            assert ns[0] == nrows + 2 * pc.depth(nw, L) and ns[-1] - 2 * L == nrows
            assert all(a - 2 * L == b for a, b in zip(ns, ns[1:]))


def test_loader_mirror_by_hand():
    # a single band of 60 rows at K = 4: rows 56 .. 59, the board, rows 0 .. 3
    ld = pc.loader(4, 60, 0, 60, True)
    assert ld.rows == [56, 57, 58, 59] + list(range(60)) + [0, 1, 2, 3] and ld.published == 68
    assert ld.crossings == 2 and ld.prewrap
    # h == K: the stream is the board three times and the counter passes h after its last row too
    ld = pc.loader(60, 60, 0, 60, True)
    assert ld.rows == list(range(60)) * 3 and ld.crossings == 3 and ld.prewrap
    # a one-row middle band at K = 4: 9 rows published, 12 issued
    ld = pc.loader(4, 60, 30, 1, True)
    assert ld.rows == list(range(26, 38)) and ld.published == 9 and ld.crossings == 0 and not ld.prewrap
    assert pc.loader_features(4, 60, 30, 1) == {"loader:n0<=12", "loader:cross=0", "loader:band=middle"}
    # the bottom band: one crossing; ghost rows instead without STEP_WRAP_Y
    assert pc.loader(4, 60, 50, 10, True).rows == list(range(46, 60)) + [0, 1, 2, 3]
    assert pc.loader(4, 60, 50, 10, True).crossings == 1
    assert pc.loader(4, 20, 10, 10, False) == pc.Load(list(range(6, 24)), 18, 0, False)
    assert pc.loader_features(4, 20, 10, 10, wrapy=False) == {"loader:n0<=18"}
    assert pc.loader_features(60, 60, 0, 60) >= {"loader:h==K", "loader:band=single", "loader:cross=2+", "loader:n0>18"}
    # every streamed row is the segment's row modulo h
    for K, h, row0, nrows in [(8, 8, 3, 1), (15, 16, 0, 16), (24, 61, 31, 30)]:
        ld = pc.loader(K, h, row0, nrows, True)
        assert ld.rows == [(row0 - K + j) % h for j in range(max(12, nrows + 2 * K))]


# ----- the loop-tail cases reach every feature -----

def brute_force(nw, L):
    """Recomputed here from stage_features alone: every feature of every role over bands of 1 .. 400 rows."""
    K, out = (nw - 1) * L, set()
    for nrows in range(1, 401):
        for st in range(nw - 1):
            role = "first" if st == 0 else "last" if st == nw - 2 else "middle"
            out |= {f"{role}:{f}" for f in pc.stage_features(L, nrows + 2 * K - 2 * st * L)}
        n0 = nrows + 2 * K
        out.add("loader:n0<=12" if n0 <= 12 else "loader:n0<=18" if n0 <= 18 else "loader:n0>18")
    return out | pc.POSITIONS


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_loop_tail_cases_cover(g):
    nw, L = g
    K = pc.depth(nw, L)
    cases = pc.loop_tail_cases(nw, L)
    want = brute_force(nw, L)
    assert want == set(pc.reachable(nw, L))
    got = set()
    for c in cases:
        assert c.H >= K and c.rows > 0 and c.H <= 124, c
        bands = wc.equal_rows_bands(c.H, c.rows)
        assert sum(n for _, n in bands) == c.H
        for row0, nrows in bands:
            got |= pc.band_features(nw, L, nrows) | pc.loader_features(K, c.H, row0, nrows)
    got.discard("loader:h==K")  # (16 x 4 on 60 rows; asserted of the small boards for every geometry)
    assert not want - got, sorted(want - got)
    assert got == want, sorted(got - want)
    assert len(cases) <= 16, cases
    # every case is needed: without it a feature is lost
    for c in cases:
        rest = pc.covered(nw, L, [x for x in cases if x != c])
        assert want - rest, f"{c} adds nothing"
    # what the issue's list of features comes to per role
    for role in pc.ROLES:
        mine = {f.split(":", 1)[1] for f in want if f.startswith(role + ":")}
        assert {f"rem={r}" for r in range(3, 21)} <= mine
        assert {"steady2plus", "tail2", "refill_full", "refill_partial1", "refill_partial2", "refill_none"} <= mine
        # (the first stage streams at least 2K + 1 rows: always a steady turn from i0 + 21 <= 2K + 1 on, always two
        # from i0 + 39 <= 2K + 1 on)
        least = 2 * K + 1 if role == "first" else 2 * L + 1
        assert ("steady0" in mine) == (least < pc.i0(L) + pc.RING + pc.QUEUE)
        assert ("steady1" in mine) == (least < pc.i0(L) + 2 * pc.RING + pc.QUEUE)
    first = {f for f in want if f.startswith("first:")}
    assert "first:short" not in first and "first:queue_partial" not in first  # n >= 2K + 1 > i0 + 3
    last = {f.split(":", 1)[1] for f in want if f.startswith("last:")}
    assert "queue_partial" in last and {"rem=1", "rem=2"} <= last
    assert ("short" in last) == (L != 3)  # L = 3: n = nrows + 6 > i0 = 6
    assert ("loader:n0<=12" in want) == (g == (5, 1)) and ("loader:n0<=18" in want) == (K <= 8)


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_small_and_ghost_cases(g):
    nw, L = g
    K = pc.depth(nw, L)
    small = pc.small_cases(nw, L)
    assert len(small) == 12 and {c.H for c in small} == {K, K + 1} and {c.W for c in small} == {64, 65, 128}
    feats = set()
    for c in small:
        assert c.rows in (1, c.H)
        for row0, nrows in wc.equal_rows_bands(c.H, c.rows):
            feats |= pc.loader_features(K, c.H, row0, nrows)
    assert "loader:h==K" in feats and "loader:cross=2+" in feats
    strips = pc.ghost_strips(nw, L)
    assert len(strips) == (3 if K <= 8 else 2) and all(s.h >= K for s in strips)
    classes = set()
    for s in strips:
        bands = wc.equal_rows_bands(s.h, s.rows)
        assert len(bands) == 2 or (K == 8 and s.h == 8 and len(bands) == 4)
        for row0, nrows in bands:
            classes |= pc.loader_features(K, s.h, row0, nrows, wrapy=False)
    assert classes == {"loader:n0>18"} | ({"loader:n0<=18"} if K <= 8 else set())
    assert min(n for _, n in wc.equal_rows_bands(strips[-1].h, strips[-1].rows)) > 40
    assert "last:steady2plus" in pc.band_features(nw, L, 41)


def test_thread_rank_geometries():
    assert sorted(L for _, L in pc.MULTI_GEOMETRIES) == [1, 2, 3, 3, 4] and pc.DEFAULT in pc.MULTI_GEOMETRIES
    assert all(2 * pc.depth(*g) <= pc.MULTI.H // 2 for g in pc.MULTI_GEOMETRIES)
    assert sorted(L for _, L in pc.GRID_GEOMETRIES) == [1, 2, 3, 4]
    assert all(2 * pc.depth(*g) <= 63 and 2 * pc.depth(*g) <= pc.GRID.H // 2 for g in pc.GRID_GEOMETRIES)
    assert all(4 * pc.depth(*g) + 3 <= pc.GENS_TOTAL for g in pc.MULTI_GEOMETRIES + pc.GRID_GEOMETRIES)
    assert pc.TALL_GEOMETRIES == [(5, 1), (5, 2), (7, 1), (9, 1)]


def test_cut_entries():
    assert pc.kernel_name(9, 3, 2) == "pipe@24(8x3,2/CU)"
    assert pc.cut(24, 9, 3) == "cut24=pipe@24(8x3,1/CU)"
    assert pc.cut(12, 7, 1) == "cut12=pipe@6(6x1,1/CU)+pipe@6(6x1,1/CU)"
    assert pc.cut(32, 9, 3, 2, (8,)) == "cut32=pipe@24(8x3,2/CU)+temporal@8"


# ----- the plans -----

@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_plans(gol, g):
    """``build_plan`` cuts every board into the bands the lists assume and covers it once."""
    nw, L = g
    K = pc.depth(nw, L)
    boards = [(c.H, wc.TAIL_W, c.rows) for c in pc.loop_tail_cases(nw, L)] + [tuple(c) for c in pc.small_cases(nw, L)]
    for H, W, rows in boards:
        waves, _ = wc.build(gol, H, W, K, "torus", rows)
        assert wc.bands_of(waves) == wc.equal_rows_bands(H, rows), (H, W, rows)
        assert wc.covers_once(waves, (0, H, 0, wc.nwords(W)))
    for s in pc.ghost_strips(nw, L):
        waves, _ = wc.build(gol, s.h, wc.TAIL_W, K, "torus", s.rows)
        assert wc.bands_of(waves) == wc.equal_rows_bands(s.h, s.rows)
        assert wc.covers_once(waves, (0, s.h, 0, wc.nwords(wc.TAIL_W)))


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_wide_plans(gol, g):
    """The wide shapes cut into two bands keep what wide_cases.SHAPES describes: per band the full-width segments and
    the remainder segment, the tail word of 3950 columns in lane 62, a seam between full-width segments on 8000."""
    K = pc.depth(*g)
    shapes = pc.wide_cases(*g)
    assert len(shapes) == sum(1 for s in wc.SHAPES if s.H >= K) >= 4
    for s in shapes:
        rows, nw = pc.wide_rows(s), wc.nwords(s.W)
        waves, _ = wc.build(gol, s.H, s.W, K, "torus", rows)
        bands = wc.equal_rows_bands(s.H, rows)
        assert len(bands) == 2 and wc.bands_of(waves) == bands and wc.covers_once(waves, (0, s.H, 0, nw))
        full = [w for w in waves if wc.is_full_width(w)]
        assert sorted((int(w.row0[0]), int(w.col[1])) for w in full) == [
            (r0, wc.SEG * i) for r0, _ in bands for i in range(s.full_per_band)]
        rest = [seg for w in waves if not wc.is_full_width(w) for seg in wc.segments(w)]
        assert sorted(rest) == ([(r0, s.full_per_band * wc.SEG, s.rest) for r0, _ in bands] if s.rest else [])
        if s is wc.S3950:
            assert all(int(w.col[62]) == nw - 1 and w.store[62] for w in full)
        if s is wc.S8000:
            assert any(int(w.col[1]) == 0 and int(w.col[63]) == wc.SEG for w in full)


def test_thread_rank_plans(gol):
    """The first pass of a two-pass superstep also stores K ghost rows each side, on a 2 x 2 grid the ghost words
    too."""
    h, W = pc.MULTI.H // 2, pc.MULTI.W
    nw = wc.nwords(W)
    for g in pc.MULTI_GEOMETRIES:
        K = pc.depth(*g)
        region = (-K, h + K, 0, nw)
        waves, _ = wc.build(gol, h, W, K, "torus", pc.MULTI_ROWS, region)
        assert wc.bands_of(waves) == [(r0 - K, n) for r0, n in wc.equal_rows_bands(h + 2 * K, pc.MULTI_ROWS)]
        assert wc.covers_once(waves, region)
    h, W = pc.GRID.H // 2, pc.GRID.W // 2
    nw = wc.nwords(W)
    for g in pc.GRID_GEOMETRIES:
        K = pc.depth(*g)
        region = (-K, h + K, -1, nw + 1)
        waves, _ = wc.build(gol, h, W, K, "torus", pc.MULTI_ROWS, region, x_wrap=False)
        assert wc.bands_of(waves) == [(r0 - K, n) for r0, n in wc.equal_rows_bands(h + 2 * K, pc.MULTI_ROWS)]
        assert wc.covers_once(waves, region)
        assert sorted({(c, n) for w in waves for _, c, n in wc.segments(w)}) == [(-1, wc.SEG), (wc.SEG - 1, 4)]
