"""Envelope mode on the CPU backend, the oracle ``numpy_envelope`` against hand-written patterns, thread ranks in 1-D
and 2-D grids, ranks that disagree, ``GOL_ENVELOPE`` / ``GOL_ENVELOPE_OUT`` and the refusals.  The cases and their
oracle-only conditions are envelope_cases.py's."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import envelope_cases as ec
import film_cases as fc
import wide_cases as wc
from gol_amd.ops import initial_board, numpy_envelope, numpy_step_rule
from gol_amd.ops.rle import pattern_cells


def _sim(gol, N, **kw):
    kw.setdefault("backend", "cpu")
    return gol.Simulation(N, **kw)


# ----- the oracle -----

def test_oracle_blinker_is_a_plus():
    b = np.zeros((5, 5), np.uint8)
    b[2, 1:4] = 1
    plus = np.zeros((5, 5), np.uint8)
    plus[2, 1:4] = 1
    plus[1:4, 2] = 1
    for bounded in (False, True):
        assert np.array_equal(numpy_envelope(b, "B3/S23", 0, bounded=bounded), b)
        for gens in (1, 2, 7):
            env, last = numpy_envelope(b, "B3/S23", gens, bounded=bounded, return_board=True)
            assert np.array_equal(env, plus) and env.sum() == 5 and env.dtype == np.uint8
            assert np.array_equal(last, b if gens % 2 == 0 else b.T)


def test_oracle_glider_track():
    """A glider's four phases by hand on an 8 x 8 torus: the envelope over 4 generations is their union, 5 cells each,
    the last the first moved one cell down and right."""
    phases = [
        [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)],
        [(1, 0), (1, 2), (2, 1), (2, 2), (3, 1)],
        [(1, 2), (2, 0), (2, 2), (3, 1), (3, 2)],
        [(1, 1), (2, 2), (2, 3), (3, 1), (3, 2)],
        [(1, 2), (2, 3), (3, 1), (3, 2), (3, 3)],
    ]
    boards = []
    for cells in phases:
        b = np.zeros((8, 8), np.uint8)
        for r, c in cells:
            b[r, c] = 1
        boards.append(b)
    for g in range(1, 5):  # (the hand-written phases are the rule's)
        assert np.array_equal(numpy_step_rule(boards[g - 1], "B3/S23", 1), boards[g]), g
    union = np.zeros((8, 8), np.uint8)
    for g, b in enumerate(boards):
        union |= b
        env, last = numpy_envelope(boards[0], "B3/S23", g, return_board=True)
        assert np.array_equal(env, union) and np.array_equal(last, b), g
    assert union.sum() == 11  # (the five five-cell phases overlap: 11 distinct cells, counted by hand)


# ----- the CPU backend -----

@pytest.mark.parametrize("N", [n for n in ec.SIZES if n <= 200])
@pytest.mark.parametrize("K", ec.DEPTHS)
def test_sweep(gol, K, N):
    ec.run_sweep_case(lambda n, **kw: _sim(gol, n, **kw), K, N, kernel="cpu")


@pytest.mark.parametrize("R", [16, 24])
def test_multipass_supersteps(gol, R):
    ec.run_multipass_case(lambda n, **kw: _sim(gol, n, **kw), R)


@pytest.mark.parametrize("K", ec.DEPTHS)
@pytest.mark.parametrize("rule", ec.NBHD_RULES)
def test_neighbourhoods(gol, rule, K):
    ec.run_nbhd_case(lambda n, **kw: _sim(gol, n, **kw), rule, K, 65)


def test_the_gpu_cases_meet_the_oracle_only_conditions():
    """The sizes, rules and seeds that only test_gpu_envelope.py runs (1000 x 1000; the neighbourhoods on 64 and 137), asked
    of the oracle here, where no GPU is needed."""
    for K in (1, 2, 8):
        for boundary in ec.BOUNDARIES:
            for rule in ec.sweep_rules(boundary):
                assert ec.lively(1000, 1000, 1000, rule, boundary, 2 * K + 1, K, ec.SWEEP_GENS), (K, rule, boundary)
    for K in ec.DEPTHS:
        for N in (64, 137):
            for rule in ec.NBHD_RULES:
                for boundary in ec.BOUNDARIES:
                    assert ec.lively(N, N, 12, rule, boundary, 2 * K + 1, K, ec.SWEEP_GENS), (K, N, rule, boundary)


@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
def test_life_cycle(gol, tmp_path, boundary):
    ec.run_life_cycle(lambda n, **kw: _sim(gol, n, **kw), tmp_path, boundary, kernel="cpu")


@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
def test_views(gol, boundary):
    ec.run_views(lambda n, **kw: _sim(gol, n, **kw), boundary, fc.WINDOWS, fc.WRAPPING)


def test_from_rle_and_load_rle(gol, tmp_path):
    """from_rle(**kw) takes envelope=True; load_rle() is init(0) and an or stamp: E is the pattern at generation 0."""
    path = tmp_path / "glider.rle"
    path.write_text("x = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n")
    s = gol.Simulation.from_rle(str(path), 16, at=(2, 2), backend="cpu", envelope=True)
    start, env = s.envelope()
    assert start == 0 and env.sum() == 5 and np.array_equal(env, s.board())
    b0 = s.board()
    s.step(8)
    ref, last = numpy_envelope(b0, "B3/S23", 8, return_board=True)
    ec.check(s, 0, ref, last)
    assert ref.sum() > 5 and not np.array_equal(ref, last)


@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
@pytest.mark.parametrize("name", list(fc.RANK_CASES))
def test_thread_ranks(gol, name, boundary):
    P, kw, H, W, windows = fc.RANK_CASES[name]
    rect = windows[0]  # (over the point where tiles meet; inside the board)
    h = ec.history(H, W, ec.RANK_SEED, ec.HIGHLIFE, boundary, ec.RANK_GENS)
    assert ec.lively(H, W, ec.RANK_SEED, ec.HIGHLIFE, boundary, ec.RANK_GENS, 8)
    parts = wc.run_ranks(gol, P, H, W, "cpu", script=ec.rank_script(rect), rule=ec.HIGHLIFE, boundary=boundary, envelope=True, **kw)
    ec.check_rank_parts(H, W, parts, h, rect)


def test_ranks_disagree(gol):
    """Every rank raises at init and none hangs."""
    P = 3
    ts = gol.parallel.thread_transports(P)
    errs = [None] * P

    def rank_main(r):
        try:
            gol.Simulation(32, ts[r], backend="cpu", envelope=r != 1).init(5)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "envelope" in str(e) and "disagree" in str(e) for e in errs), errs


def test_option_and_refusals(gol, monkeypatch):
    monkeypatch.delenv("GOL_ENVELOPE", raising=False)
    plain = gol.Simulation(16, backend="cpu").init(5)
    assert plain.stats()["envelope"] is None and plain.config.envelope is False
    for call in (plain.envelope, lambda: plain.envelope_window(0, 0, 4, 4), lambda: plain.envelope_density(8, 64),
                 plain.envelope_population, plain.envelope_clear):
        with pytest.raises(ValueError) as e:
            call()
        assert "envelope mode" in str(e.value) and "envelope=True" in str(e.value)
    for call in (plain.engine.envelope, lambda: plain.engine.envelope_window(0, 0, 4, 4),
                 lambda: plain.engine.envelope_density(8, 64), plain.engine.envelope_population, plain.engine.envelope_clear):
        with pytest.raises(gol.native.GolError) as e:  # the engine on its own
            call()
        assert "envelope mode" in str(e.value)
    monkeypatch.setenv("GOL_ENVELOPE", "1")  # read per call
    assert gol.Simulation(16, backend="cpu").init(5).stats()["envelope"] == 0
    monkeypatch.setenv("GOL_ENVELOPE", "0")
    assert gol.Simulation(16, backend="cpu").stats()["envelope"] is None
    monkeypatch.delenv("GOL_ENVELOPE")
    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"film": (0, 0, 8, 8)}, "film"),
                     ({"density_film": (8, 64)}, "density_film"), ({"compat": True}, "compat"), ({"subtiles": 2}, "subtiles=2")]:
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="cpu", envelope=True, **kw)
        assert word in str(e.value) and "envelope" in str(e.value), str(e.value)
    s = gol.Simulation(64, backend="cpu", envelope=True, boundary="dead").init(5)
    with pytest.raises(ValueError) as e:
        s.envelope_window(60, 0, 8, 8)
    assert "inside the bounded 64 x 64" in str(e.value)
    with pytest.raises(ValueError):
        s.envelope_density(8, 65)


def test_engine_refusals(gol):
    """The engine on its own: the same refusals from EngineConfig, each naming both modes."""
    dec = gol.native.make_decomposition(64, 1, False, "1d", "", 0)
    geo = gol.native.make_geometry(dec, 0)
    for attr, value, word in [("census", True, "census"), ("signature", True, "signature"), ("film", (0, 0, 8, 8), "film"),
                              ("density_film", (8, 64), "density_film"), ("compat", True, "GOL_COMPAT"),
                              ("subtiles", 2, "GOL_SUBTILES=2")]:
        cfg = gol.native.EngineConfig()
        cfg.backend = "cpu"
        cfg.envelope = True
        setattr(cfg, attr, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
        assert word in str(e.value) and "envelope" in str(e.value), str(e.value)


# ----- the CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_BOUNDARY",
              "GOL_PATTERN_FILE", "GOL_PATTERN_AT", "GOL_RLE_OUT", "GOL_CENSUS", "GOL_CENSUS_OUT", "GOL_COMPAT", "GOL_SUBTILES",
              "GOL_SIGNATURE", "GOL_SIGNATURE_OUT", "GOL_FILM", "GOL_FILM_OUT", "GOL_DENSITY_FILM", "GOL_DENSITY_FILM_OUT",
              "GOL_ENVELOPE", "GOL_ENVELOPE_OUT", "GOL_SOUPS"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
def test_cli_envelope_out(gol, gol_bin, tmp_path, P, boundary):
    """GOL_ENVELOPE_OUT implies the mode; the file goes through parse_rle and equals the oracle's envelope; GOL_RLE_OUT
    beside it still holds the final board."""
    N, gens, rule = 48, 13, "B36/S23"
    H = N * P
    r = _cli(gol_bin, [5, N, gens, 64, 0], tmp_path, GOL_ENVELOPE_OUT=tmp_path / "env.rle", GOL_RLE_OUT=tmp_path / "end.rle",
             GOL_NRANKS=P, GOL_RULE=rule, GOL_BOUNDARY=boundary, GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    ref, last = numpy_envelope(initial_board(5, N, P, True), rule, gens, bounded=boundary == "dead", return_board=True)
    assert not np.array_equal(ref, last) and not ref.all()

    def cells_of(path):
        p = gol.native.parse_rle(path.read_text())
        assert p.rule == rule and (p.rows, p.cols) == (H, N)
        assert p.topology == ("P" if boundary == "dead" else "")
        return pattern_cells(p)

    assert np.array_equal(cells_of(tmp_path / "env.rle"), ref)
    assert np.array_equal(cells_of(tmp_path / "end.rle"), last)
    assert json.loads((tmp_path / "m.json").read_text())["envelope"] == 0


def test_cli_flag_alone_and_default(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "a", GOL_ENVELOPE=1, GOL_METRICS_JSON=tmp_path / "a" / "m.json")
    assert r.returncode == 0, r.stderr
    assert json.loads((tmp_path / "a" / "m.json").read_text())["envelope"] == 0
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "b", GOL_METRICS_JSON=tmp_path / "b" / "m.json")
    assert r.returncode == 0, r.stderr
    assert json.loads((tmp_path / "b" / "m.json").read_text())["envelope"] is None


@pytest.mark.parametrize("P", [1, 3])
def test_cli_unwritable_path(gol_bin, tmp_path, P):
    bad = tmp_path / "no" / "such" / "dir" / "env.rle"
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_ENVELOPE_OUT=bad, GOL_NRANKS=P)
    assert r.returncode != 0 and str(bad) in r.stderr and "GOL_ENVELOPE_OUT" in r.stderr


@pytest.mark.parametrize("env,word", [({"GOL_COMPAT": "reference"}, "GOL_COMPAT"), ({"GOL_SUBTILES": 2}, "GOL_SUBTILES=2"),
                                      ({"GOL_CENSUS": 1}, "census"), ({"GOL_SIGNATURE": 1}, "signature"),
                                      ({"GOL_FILM": "0,0,8,8"}, "film"), ({"GOL_DENSITY_FILM": "8,64"}, "density_film"),
                                      ({"GOL_SOUPS": 4}, "GOL_SOUPS")],
                         ids=["compat", "subtiles", "census", "signature", "film", "density_film", "soups"])
def test_cli_refusals(gol_bin, tmp_path, env, word):
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_ENVELOPE=1, **env)
    assert r.returncode != 0 and word in r.stderr and "envelope" in r.stderr, r.stderr


def test_cli_envelope_out_too_many_cells(gol_bin, tmp_path):
    """More than 2^26 cells is refused before the run, as GOL_RLE_OUT refuses them."""
    r = _cli(gol_bin, [5, 8200, 1, 64, 0], tmp_path, GOL_ENVELOPE_OUT=tmp_path / "env.rle")
    assert r.returncode != 0 and "GOL_ENVELOPE_OUT" in r.stderr and "2^26" in r.stderr
    assert not (tmp_path / "env.rle").exists()
