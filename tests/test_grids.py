"""2-D rank grids beyond 2 x 2 on the CPU backend: 3 x 3, 4 x 2, 2 x 4 and Px x 1 (the cases of grid_cases.py), as
thread ranks, bit for bit against the numpy oracles on the assembled global board.

2 x 2 is the degenerate grid: a rank's E and W neighbours are one rank, N and S are one rank, all four corner
neighbours are one rank, and every rank touches two edges of a bounded board.  Here a rank has eight distinct
neighbours (3 x 3), or x neighbours only (Px x 1), tiles differ in height and width within one job, a bounded board
has a centre rank and edge-only ranks, the census is owned under real corner neighbours, and windows, density blocks
and stamps span four and nine ranks.  A neighbour table that swaps NW with NE and SW with SE (consistently for send
and receive, so nothing deadlocks) passes every 2 x 2 test; it fails here on the 3 x 3 and 4 x 2 grids with tiles of
two words or more."""
import numpy as np
import pytest

import grid_cases as gc
from grid_cases import B1, CASES, CONWAY, HIGHLIFE, case_id

BOUNDARIES = ["torus", "dead"]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_torus(gol, case):
    for rule in (CONWAY, HIGHLIFE):
        parts = gc.run_ranks(gol, case, "cpu", rule=rule)
        gc.check_board(case, parts, gc.board_after(case, rule, "torus"))
        for p in parts:
            assert p.stats["depth"] == gc.halo_depth_of(case) and p.stats["exchanges"] == gc.exchanges_of(case), p.stats


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bounded(gol, case):
    for rule in (HIGHLIFE, B1):
        ref = gc.board_after(case, rule, "dead")
        assert not np.array_equal(ref, gc.board_after(case, rule, "torus")), "the input does not tell the boundaries apart"
        parts = gc.run_ranks(gol, case, "cpu", rule=rule, boundary="dead")
        gc.check_board(case, parts, ref)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_census(gol, case, boundary):
    """Every rank gets the same, global series; no rank counts a ghost cell of one of its (distinct) neighbours."""
    for rule in (HIGHLIFE, B1):
        parts = gc.run_ranks(gol, case, "cpu", script=gc.census_script, rule=rule, boundary=boundary, census=True)
        gc.check_census(case, parts, rule, boundary)


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_views(gol, boundary):
    """Windows, density maps and stamps over four and nine ranks of the 3 x 3 grid: every rank's result is numpy's,
    and so is one rank's holding the whole board."""
    bounded = boundary == "dead"
    want = gc.views_expected(bounded)
    parts = gc.run_ranks(gol, gc.VIEW_CASE, "cpu", script=gc.views_script(bounded), boundary=boundary)
    for p in parts:
        gc.check_views(p.result, want, f"rank {p.rank} (cx {p.cx}, cy {p.cy})")
    gc.check_board(gc.VIEW_CASE, parts, want["stepped"])
    one = gol.Simulation(gc.VIEW_CASE.H, backend="cpu", width=gc.VIEW_CASE.W, boundary=boundary).init(5, seed=gc.SEED)
    gc.check_views(gc.views_script(bounded)(one), want, "one rank")


def test_mismatch_report_names_the_halo_item():
    """The report counts a wrong cell under its tile, and under the rows, the word and the corner block it lies in."""
    case = CASES[0]
    ref = gc.start_board(case)
    parts = [gc.Part(0, 1, 1, 67, 192, ref[67:134, 192:320], {}, None), gc.Part(1, 2, 1, 67, 320, ref[67:134, 320:448], {}, None)]
    assert gc.mismatch_report(parts, ref, ref) == ""
    got = ref.copy()
    got[67, 192] ^= 1    # rank 0: first row, first word -> the NW corner block
    got[100, 319] ^= 1   # rank 0: a middle row, the last word (of two) -> E only
    got[133, 384] ^= 1   # rank 1: the last row, the last word -> a corner block
    got[90, 330] ^= 1    # rank 1: a middle row of the first word -> W only
    got[70, 200] ^= 1    # rank 0 again: rows and word, so the corner block too
    lines = gc.mismatch_report(parts, got, ref).splitlines()
    assert lines[0].startswith("5 of ")
    assert "rank 0 (cx 1, cy 1; rows 67..133, columns 192..319): 3 wrong, 2 in the first/last 16 rows, 3 in the " \
           "first/last word, 2 in the corner blocks" in lines[1]
    assert "rank 1 (cx 2, cy 1; rows 67..133, columns 320..447): 2 wrong, 1 in the first/last 16 rows, 2 in the " \
           "first/last word, 1 in the corner blocks" in lines[2]
