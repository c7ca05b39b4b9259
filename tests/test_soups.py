"""Soup batches on the CPU backend, the oracle ``numpy_soup_settle``, the refusals and the ``GOL_SOUPS`` CLI mode.

The cases are soup_cases.py's, shared with test_gpu_soups.py: plain stepping bit for bit, seam patterns from arrays,
random soups that settle (all four result arrays and the boards against the oracle), soups that do not, independence of
the chunk and of resumption, mixed settling times in one batch; at 128^2 and 256^2 the sparse, placed and tiled boards
that settle within the oracle's reach, so the m = 2 and m = 4 paths of soups_cpu.cpp (the GPU tests' second reference)
are themselves checked against the oracle, and max_gens on the generation of the hit.  Every comparison is exact."""
import os

import numpy as np
import pytest

import soup_cases as sc
from gol_amd.ops import initial_board, numpy_soup_settle, numpy_step, numpy_step_rule
from gol_amd.utils import read_dump
from test_cli import BANNER, run  # the CLI helper of tests/test_cli.py (CPU backend, launcher variables cleared)

BACKEND = "cpu"


# ---- the oracle itself ----------------------------------------------------------------------------------------------

def test_oracle_schedule_and_transient():
    """The oracle on boards whose answer is known by hand: a blinker (period 2: saved at generation 1, hit at 3), a
    still life, a board that dies (transient 1 into the empty board's period 1), and an unsettled run."""
    b = np.zeros((64, 64), dtype=np.uint8)
    b[5, 4:7] = 1
    assert numpy_soup_settle(b, "B3/S23", 100, True)[:4] == (2, 0, 3, 3)
    blk = np.zeros((64, 64), dtype=np.uint8)
    blk[8:10, 8:10] = 1
    assert numpy_soup_settle(blk, "B3/S23", 100, True)[:4] == (1, 0, 1, 4)
    dot = np.zeros((64, 64), dtype=np.uint8)
    dot[3, 3] = 1
    p, t, g, pop, last = numpy_soup_settle(dot, "B3/S23", 100, True)
    assert (p, t, g, pop) == (1, 1, 2, 0) and not last.any()  # saved at 1 (empty), hit at 2
    p, t, g, pop, last = numpy_soup_settle(sc.soup(64, sc.SEED), "B2/S", 40, True)
    assert (p, t, g) == (0, -1, 40) and np.array_equal(last, numpy_step_rule(sc.soup(64, sc.SEED), "B2/S", 40))
    assert pop == int(last.sum())


# ---- the cases on the CPU backend -----------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", sc.STEP_RULES)
@pytest.mark.parametrize("S", [64, 128])
def test_plain_steps(gol, S, rule):
    sc.check_plain_steps(gol, BACKEND, S, rule)


def test_plain_steps_256(gol):
    sc.check_plain_steps(gol, BACKEND, 256, "B36/S23")


@pytest.mark.parametrize("S", sc.SIZES)
def test_seam_patterns(gol, S):
    sc.check_patterns(gol, BACKEND, S)


@pytest.mark.parametrize("rule", sc.FAMILY_RULES)
@pytest.mark.parametrize("S", sc.SIZES)
def test_three_families_settle(gol, S, rule):
    """Sparse, placed and tiled boards in one batch: the m = 2 and m = 4 paths of soups_cpu.cpp against the oracle."""
    sc.check_variant(gol, BACKEND, S, rule)


@pytest.mark.parametrize("S,rule", sc.FAMILY_CHUNKS)
def test_family_chunks_and_resumption(gol, S, rule):
    sc.check_family_chunks(gol, BACKEND, S, rule)


def test_mixed_settling_times_256(gol):
    sc.check_mixed(gol, BACKEND, chunk=512, S=256)


def test_max_gens_on_the_hit(gol):
    sc.check_max_gens_edges(gol, BACKEND)


@pytest.mark.parametrize("S,rule,n", sc.SETTLING)
def test_random_soups_settle(gol, S, rule, n):
    sc.check_settling(gol, BACKEND, S, rule, n)


def test_soups_that_do_not_settle(gol):
    sc.check_unsettled(gol, BACKEND)


@pytest.mark.parametrize("S,rule,n", sc.SETTLING[:2])
def test_chunk_independence_and_resumption(gol, S, rule, n):
    sc.check_chunks(gol, BACKEND, S, rule, n)


def test_mixed_settling_times(gol):
    sc.check_mixed(gol, BACKEND)


def test_result_types_and_stats(gol):
    sb = gol.SoupBatch(3, backend=BACKEND, seed=sc.SEED)
    res = sb.settle(50)
    assert res._fields == ("period", "transient", "generation", "population")
    assert [a.dtype for a in res] == [np.uint32, np.int64, np.uint32, np.uint32]
    st = sb.stats()
    assert st["kernel"] == "soups@64" and st["launches"] == 1 and st["settled"] == 0 and st["backend"] == "cpu"
    assert sb.boards([2, 0]).shape == (2, 64, 64) and np.array_equal(sb.boards([2])[0], sb.boards()[2])
    # the seed wraps mod 2^64: soup 1 of seed 2^64 - 1 is seed 0's board
    wrap = gol.SoupBatch(2, backend=BACKEND, seed=(1 << 64) - 1)
    assert np.array_equal(wrap.boards([1])[0], sc.soup(64, 0))


def test_step_then_settle_counts_from_there(gol):
    """A search begun after step(g) saves at g + 2^k - 1: the oracle on the board of generation g, shifted by g."""
    g = 10
    sb = gol.SoupBatch(2, backend=BACKEND, seed=sc.SEED).step(g)
    res = sb.settle(sc.MAX_GENS, transient=True)
    for i in range(2):
        o = numpy_soup_settle(numpy_step_rule(sc.soup(64, sc.SEED + i), "B3/S23", g), "B3/S23", sc.MAX_GENS - g, True)
        assert (res.period[i], res.transient[i], res.generation[i], res.population[i]) == (o[0], o[1], o[2] + g, o[3])
    with pytest.raises(Exception, match="after settle"):
        sb.step(1)


# ---- refusals -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize(
    "kw,word",
    [
        (dict(n=4, size=96), "96"),
        (dict(n=4, size=32), "32"),
        (dict(n=0), "n = 0"),
        (dict(n=(1 << 20) + 1), "1048577"),
        (dict(n=2, rule="B13/S13V"), "B13/S13V"),
        (dict(n=2, rule="B2/S34H"), "B2/S34H"),
        (dict(n=2, rule="B03/S23"), "B03/S23"),
        (dict(n=2, boundary="dead"), "dead"),
        (dict(n=2, compat=True), "compat"),
        (dict(n=2, backend="cuda"), "cuda"),
    ],
)
def test_constructor_refusals(gol, kw, word):
    kw.setdefault("backend", BACKEND)
    with pytest.raises(ValueError, match=word):
        gol.SoupBatch(**kw)


def test_call_refusals(gol):
    sb = gol.SoupBatch(2, backend=BACKEND, seed=sc.SEED)
    with pytest.raises(ValueError, match="chunk = 0"):
        sb.settle(100, chunk=0)
    with pytest.raises(ValueError, match="chunk = -3"):
        sb.settle(100, chunk=-3)
    sb.settle(100)
    with pytest.raises(ValueError, match="max_gens = 99"):
        sb.settle(99)
    with pytest.raises(ValueError, match="index 2"):
        sb.boards([0, 2])
    assert np.array_equal(sb.records().generation, [100, 100])  # nothing ran


def test_board_array_refusals(gol):
    ok = np.zeros((2, 64, 64), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"\(64, 64\)"):
        gol.SoupBatch.from_boards(ok[0], backend=BACKEND)
    with pytest.raises(ValueError, match=r"\(2, 64, 128\)"):
        gol.SoupBatch.from_boards(np.zeros((2, 64, 128), dtype=np.uint8), backend=BACKEND)
    with pytest.raises(ValueError, match="96"):
        gol.SoupBatch.from_boards(np.zeros((2, 96, 96), dtype=np.uint8), backend=BACKEND)
    bad = ok.copy()
    bad[1, 5, 7] = 2
    with pytest.raises(ValueError, match="is 2"):
        gol.SoupBatch.from_boards(bad, backend=BACKEND)
    with pytest.raises(ValueError, match="0.5"):
        gol.SoupBatch.from_boards(ok.astype(np.float64) + 0.5, backend=BACKEND)


# ---- CLI ------------------------------------------------------------------------------------------------------------

def test_cli_csv(gol_bin, tmp_path):
    n = 8
    out = tmp_path / "soups.csv"
    r = run(gol_bin, [5, 64, sc.MAX_GENS, 256, 0], tmp_path,
            env={"GOL_SOUPS": str(n), "GOL_SOUPS_TRANSIENT": "1", "GOL_SOUPS_OUT": str(out), "GOL_SEED": str(sc.SEED)})
    assert r.returncode == 0, r.stderr
    line = r.stdout.splitlines()
    assert len(line) == 1 and line[0].startswith(f"soups {n} settled {n} of {n} in ") and line[0].endswith(" s")
    assert out.read_text().splitlines() == sc.csv_lines(sc.settling_oracles(64, "B3/S23", n))


def test_cli_rule_chunk_and_no_transient(gol_bin, tmp_path):
    n = 4
    out = tmp_path / "soups.csv"
    r = run(gol_bin, [5, 64, sc.MAX_GENS, 256, 0], tmp_path,
            env={"GOL_SOUPS": str(n), "GOL_SOUPS_OUT": str(out), "GOL_SEED": str(sc.SEED), "GOL_RULE": "B36/S23",
                 "GOL_SOUPS_CHUNK": "100"})
    assert r.returncode == 0, r.stderr
    want = [(o[0], -1, o[2], o[3]) for o in sc.settling_oracles(64, "B36/S23", n)]
    assert out.read_text().splitlines() == sc.csv_lines(want)


@pytest.mark.parametrize(
    "args,env,reason",
    [
        ([4, 64, 10, 256, 0], {}, "pattern 4"),
        ([5, 64, 10, 256, 0], {"GOL_NRANKS": "2"}, "one rank"),
        ([5, 64, 10, 256, 0], {"WORLD_SIZE": "2", "RANK": "0"}, "one rank"),
        ([5, 64, 10, 256, 0], {"GOL_BOUNDARY": "dead"}, "GOL_BOUNDARY=dead"),
        ([5, 64, 10, 256, 0], {"GOL_COMPAT": "reference"}, "GOL_COMPAT"),
        ([5, 64, 10, 256, 0], {"GOL_CENSUS": "1"}, "census"),
        ([5, 64, 10, 256, 0], {"GOL_SIGNATURE": "1"}, "signature"),
        ([5, 64, 10, 256, 0], {"GOL_FILM": "0,0,8,8"}, "film"),
        ([5, 64, 10, 256, 0], {"GOL_DENSITY_FILM": "8,64"}, "density-film"),
        ([5, 96, 10, 256, 0], {}, "size 96"),
        ([5, 64, 10, 256, 0], {"GOL_SOUPS": "0"}, "n = 0"),
        ([5, 64, 10, 256, 0], {"GOL_RULE": "B2/S34H"}, "B2/S34H"),
        ([5, 64, 10, 256, 0], {"GOL_SOUPS_CHUNK": "0"}, "chunk = 0"),
        ([5, 64, 10, 256, 0], {"GOL_SOUPS_OUT": "/nonexistent-dir/soups.csv"}, "cannot write"),
    ],
)
def test_cli_refusals(gol_bin, tmp_path, args, env, reason):
    e = {"GOL_SOUPS": "4"}
    e.update(env)
    r = run(gol_bin, args, tmp_path, env=e)
    assert r.returncode != 0
    assert reason in r.stderr, r.stderr
    assert not list(tmp_path.glob("Rank_*"))


def test_cli_unchanged_without_gol_soups(gol_bin, tmp_path):
    """GOL_SOUPS unset (or empty): the reference run, as tests/test_cli.py has it."""
    for env in (None, {"GOL_SOUPS": ""}):
        r = run(gol_bin, [5, 64, 10, 64, 1], tmp_path, env=env)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines(keepends=True)
        assert len(lines) == 2 and lines[1] == BANNER
        assert lines[0].startswith("TOTAL DURATION : ") and lines[0].endswith(", number of cell updates = 40960\n")
        _, _, cells = read_dump(os.path.join(tmp_path, "Rank_0_of_1.txt"))
        assert np.array_equal(cells, numpy_step(initial_board(5, 64, 1, True), 10))
