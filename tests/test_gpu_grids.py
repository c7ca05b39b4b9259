"""2-D rank grids beyond 2 x 2 on the HIP backend: 3 x 3, 4 x 2, 2 x 4 and Px x 1 (the cases of grid_cases.py) as
thread ranks sharing one GPU through the RCCL-semantics transport (p2p emulation: device buffers, stream-ordered
rendezvous copies, per-peer FIFO matching), bit for bit against the numpy oracles on the assembled global board.

On a 2 x 2 grid a rank's E and W neighbours are one rank, N and S are one rank, the four corner neighbours are one
rank and every rank touches two edges of the board.  What runs only here: a rank whose eight neighbours are eight
ranks (the pack / unpack copy lists, post(), the FIFO matching with 8 peers), a rank with x neighbours and no y
neighbours (regions() with e = 0 and xe = 1, no corner items), tiles of different nw and h in one job, the row and
column masks of step_rule_bounded on a centre rank and on edge-only ranks, step_census's owned-cell masks under
real corner neighbours, and window / density / stamp rectangles that span four and nine ranks.

A wrong board fails with grid_cases.mismatch_report: per rank the wrong cells, and how many lie in the first / last
16 rows, in the first / last word and in the corner blocks -- which halo item is wrong."""
import os
import subprocess

import numpy as np
import pytest

import grid_cases as gc
from grid_cases import B1, CASES, CONWAY, HIGHLIFE, case_id, pick
from gol_amd.ops import initial_board, numpy_step

pytestmark = pytest.mark.gpu

BOUNDARIES = ["torus", "dead"]


@pytest.fixture(autouse=True)
def _no_spinup(monkeypatch):
    monkeypatch.setenv("GOL_SPINUP_MS", "0")


def check_supersteps(case, parts):
    """Every rank ran at the one clamped halo depth and exchanged once per superstep: 16 + 16 + 8 is 3 exchanges."""
    for p in parts:
        assert p.stats["depth"] == gc.halo_depth_of(case), (p.rank, p.stats)
        assert p.stats["exchanges"] == gc.exchanges_of(case), (p.rank, p.stats)


# ----- B3/S23: the specialised kernels -----

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conway_auto(gol, case):
    parts = gc.run_ranks(gol, case, "hip", kernel="auto")
    gc.check_board(case, parts, gc.board_after(case, CONWAY, "torus"))
    check_supersteps(case, parts)  # (3 exchanges; 7 on the 20-row board, whose depth clamps to 6)


@pytest.mark.parametrize("schedule", ["full", "split"])
@pytest.mark.parametrize("kernel", ["temporal", "tile"])
@pytest.mark.parametrize("case", pick(1, 4, 5), ids=case_id)
def test_conway_forced(gol, case, kernel, schedule):
    parts = gc.run_ranks(gol, case, "hip", kernel=kernel, schedule=schedule)
    for p in parts:
        assert p.stats["schedule"] == schedule and p.stats["kernel"].startswith(kernel), (p.rank, p.stats)
        assert p.stats["exchanges"] == 3, (p.rank, p.stats)
    check_supersteps(case, parts)
    gc.check_board(case, parts, gc.board_after(case, CONWAY, "torus"))


def test_conway_pipe(gol, monkeypatch):
    """step_pipe on ranks with x neighbours (its passes also store the ghost words): 4 stages of 2 generations, the
    shared pass depth of 8."""
    case = CASES[0]
    monkeypatch.setenv("GOL_PIPE", "5,2,2")
    parts = gc.run_ranks(gol, case, "hip", kernel="pipe", schedule="full")
    for p in parts:
        assert p.stats["schedule"] == "full" and p.stats["kernel"].startswith("pipe@8"), (p.rank, p.stats)
    check_supersteps(case, parts)
    gc.check_board(case, parts, gc.board_after(case, CONWAY, "torus"))


# ----- step_rule, step_rule_bounded, step_census -----

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rule(gol, case):
    parts = gc.run_ranks(gol, case, "hip", rule=HIGHLIFE)
    for p in parts:
        assert p.stats["kernel"].startswith("rule@"), (p.rank, p.stats)
    check_supersteps(case, parts)
    gc.check_board(case, parts, gc.board_after(case, HIGHLIFE, "torus"))


@pytest.mark.parametrize("rule", [HIGHLIFE, B1])
@pytest.mark.parametrize("case", pick(1, 2, 4, 5, 6), ids=case_id)
def test_bounded(gol, case, rule):
    ref = gc.board_after(case, rule, "dead")
    assert not np.array_equal(ref, gc.board_after(case, rule, "torus")), "the input does not tell the boundaries apart"
    parts = gc.run_ranks(gol, case, "hip", rule=rule, boundary="dead")
    for p in parts:
        assert p.stats["kernel"].startswith("rule@") and p.stats["boundary"] == "dead", (p.rank, p.stats)
    got = gc.check_board(case, parts, ref)
    if case == CASES[0]:  # against the CPU backend on the same grid
        cpu = gc.run_ranks(gol, case, "cpu", rule=rule, boundary="dead")
        assert np.array_equal(got, gc.assemble(case, cpu)), gc.mismatch_report(parts, got, gc.assemble(case, cpu))


@pytest.mark.parametrize("rule", [HIGHLIFE, B1])
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("case", pick(1, 5, 6), ids=case_id)
def test_census(gol, case, boundary, rule):
    parts = gc.run_ranks(gol, case, "hip", script=gc.census_script, rule=rule, boundary=boundary, census=True)
    for p in parts:
        assert p.stats["kernel"].startswith("census@") and p.stats["census"] is True, (p.rank, p.stats)
    gc.check_census(case, parts, rule, boundary)


# ----- window(), density() and stamp() over four and nine ranks -----

@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_views(gol, boundary):
    """Every rank's result is numpy's and the CPU backend's."""
    bounded = boundary == "dead"
    want = gc.views_expected(bounded)
    parts = gc.run_ranks(gol, gc.VIEW_CASE, "hip", script=gc.views_script(bounded), boundary=boundary)
    cpu = gc.views_script(bounded)(
        gol.Simulation(gc.VIEW_CASE.H, backend="cpu", width=gc.VIEW_CASE.W, boundary=boundary).init(5, seed=gc.SEED))
    gc.check_views(cpu, want, "the CPU backend")
    for p in parts:
        who = f"rank {p.rank} (cx {p.cx}, cy {p.cy})"
        gc.check_views(p.result, want, who)
        gc.check_views(p.result, cpu, who)
    gc.check_board(gc.VIEW_CASE, parts, want["stepped"])


# ----- the gol program: 2-D dumps routed point to point from HIP tiles -----

def test_cli_3x3_dumps(gol_bin, tmp_path):
    P, N, gens = 9, 192, 40
    dumps = {}
    for backend in ("hip", "cpu"):
        e = dict(os.environ)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_BOUNDARY", "GOL_CENSUS",
                  "GOL_KERNEL", "GOL_SCHEDULE", "GOL_HALO_DEPTH", "GOL_KERNEL_DEPTH", "GOL_TRANSPORT"):
            e.pop(k, None)
        e.update(GOL_NRANKS=str(P), GOL_GLOBAL="1", GOL_DECOMP="2d", GOL_GRID="3x3", GOL_BACKEND=backend)
        cwd = tmp_path / backend
        cwd.mkdir()
        r = subprocess.run([gol_bin, "5", str(N), str(gens), "256", "1"], cwd=cwd, env=e, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        dumps[backend] = {f.name: f.read_bytes() for f in sorted(cwd.glob("Rank_*"))}
    assert sorted(dumps["hip"]) == [f"Rank_{r}_of_{P}.txt" for r in range(P)] == sorted(dumps["cpu"])
    for name, data in dumps["hip"].items():
        assert data == dumps["cpu"][name], name
    from gol_amd.utils import read_dump

    parts = sorted((read_dump(str(tmp_path / "hip" / name))[1:] for name in dumps["hip"]), key=lambda t: t[0])
    assert np.array_equal(np.vstack([cells for _, cells in parts]), numpy_step(initial_board(5, N, P, False), gens))
