"""Film mode on the CPU backend, the oracle and the CLI: per-generation frames of a board window (``film=(r0, c0, rows,
cols)``, ``Simulation.film()``) against ``numpy_film``; the depth and size sweep up to 200 cells a side, the window
shapes, the start / clear / restart rules, thread ranks in 1-D and 2-D grids, ranks that disagree, ``numpy_film``
against a literal per-cell loop, ``GOL_FILM_OUT`` and the refusals."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import film_cases as fc
import wide_cases as wc
from gol_amd.ops import initial_board, numpy_film, parse_rule, random_board


def _sim(gol, N, **kw):
    kw.setdefault("backend", "cpu")
    return gol.Simulation(N, **kw)


@pytest.mark.parametrize("N", [n for n in fc.SIZES if n <= 200])
@pytest.mark.parametrize("K", fc.DEPTHS)
def test_sweep(gol, K, N):
    fc.run_sweep_case(lambda n, **kw: _sim(gol, n, **kw), K, N, kernel="cpu")


@pytest.mark.parametrize("K", [8, 3])
@pytest.mark.parametrize("name", list(fc.WINDOWS))
def test_window_shapes(gol, name, K):
    fc.run_window_case(lambda n, **kw: _sim(gol, n, **kw), name, K)


def test_numpy_film_against_a_per_cell_loop():
    """The oracle itself, cell by cell on a 7 x 130 board: both boundaries, a window across both seams."""
    H, W, gens, rule = 7, 130, 6, "B36/S23"
    birth, survive = parse_rule(rule)
    for bounded in (False, True):
        rect = (2, 60, 4, 12) if bounded else (5, 125, 6, 20)
        b = random_board(H, W, 4).astype(np.uint8)
        got = numpy_film(b, rule, gens, rect, bounded=bounded)
        assert got.shape == (gens, rect[2], rect[3]) and got.dtype == np.uint8
        for g in range(gens):
            nxt = np.zeros_like(b)
            for y in range(H):
                for x in range(W):
                    n = 0
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if dy == 0 and dx == 0:
                                continue
                            yy, xx = y + dy, x + dx
                            if bounded:
                                if 0 <= yy < H and 0 <= xx < W:
                                    n += int(b[yy, xx])
                            else:
                                n += int(b[yy % H, xx % W])
                    nxt[y, x] = ((survive if b[y, x] else birth) >> n) & 1
            b = nxt
            for i in range(rect[2]):
                for j in range(rect[3]):
                    assert got[g, i, j] == b[(rect[0] + i) % H, (rect[1] + j) % W], (bounded, g, i, j)
        assert len({f.tobytes() for f in got}) >= 2


def test_start_clear_restart_rules(gol, tmp_path):
    """Several step() calls around a stamp(), set_board(), film_clear(), checkpoint() / restore() and init()."""
    N, rule, rect, seed = 137, fc.HIGHLIFE, (100, 120, 50, 40), 8
    s = _sim(gol, N, rule=rule, halo_depth=8, film=rect).init(5, seed=seed)
    assert s.film()[0] == 0 and s.film()[1].shape == (0, 50, 40)
    ref = fc.frames_of(N, N, seed, rule, "torus", 29, rect)
    boards = fc.boards_of(N, N, seed, rule, "torus", 29)
    s.step(5).step(20).step(1)
    fc.check(s, 0, ref[:26], boards[25], rect)
    s.film_clear()
    assert s.film()[0] == 26 and len(s.film()[1]) == 0
    s.step(3)
    fc.check(s, 26, ref[26:], boards[28], rect)
    # stamp() and set_board() leave the record running
    s.stamp(np.ones((3, 3), np.uint8), at=(110, 130), mode="xor")
    b = s.board()
    s.set_board(b)
    s.step(4)
    start, got = s.film()
    assert start == 26 and len(got) == 7 and np.array_equal(got[:3], ref[26:])
    assert np.array_equal(got[3:], numpy_film(b, rule, 4, rect))
    # checkpoint / restore: the record restarts at the restored generation
    s.checkpoint(str(tmp_path / "ck"))
    s.step(2)
    assert s.restore(str(tmp_path / "ck")) == 33
    assert s.film()[0] == 33 and len(s.film()[1]) == 0
    s.step(5)
    start, got = s.film()
    assert start == 33 and np.array_equal(got, numpy_film(numpy_film(b, rule, 4, (0, 0, N, N))[-1], rule, 5, rect))
    # init() starts it at 0
    s.init(5, seed=seed)
    s.step(7)
    fc.check(s, 0, ref[:7], boards[6], rect)


@pytest.mark.parametrize("boundary", fc.BOUNDARIES)
@pytest.mark.parametrize("name", ["1d3", "2x2", "3x3"])
def test_thread_ranks(gol, name, boundary):
    P, kw, H, W, _ = fc.RANK_CASES[name]
    for rect in fc.rank_windows(name, boundary):
        ref, board = fc.rank_ref(name, fc.HIGHLIFE, boundary, rect)
        assert fc.distinct(H, W, fc.RANK_SEED, fc.HIGHLIFE, boundary, fc.RANK_GENS, rect)
        assert boundary == "torus" or fc.told_apart(H, W, fc.RANK_SEED, fc.HIGHLIFE, fc.RANK_GENS, (0, 0, H, W))
        parts = wc.run_ranks(gol, P, H, W, "cpu", script=fc.film_script, rule=fc.HIGHLIFE, boundary=boundary, film=rect, **kw)
        assert np.array_equal(wc.assemble(H, W, parts), board)
        for p in parts:  # every rank gets every frame
            start, frames, st = p.result
            assert start == 0 and st["film"] == rect and np.array_equal(frames, ref), p.rank


@pytest.mark.parametrize("films", [[(0, 0, 8, 8), None, (0, 0, 8, 8)], [(0, 0, 8, 8), (0, 1, 8, 8), (0, 0, 8, 8)]],
                         ids=["mode", "rectangle"])
def test_ranks_disagree(gol, films):
    """Every rank raises at init and none hangs."""
    P = 3
    ts = gol.parallel.thread_transports(P)
    errs = [None] * P

    def rank_main(r):
        try:
            gol.Simulation(32, ts[r], backend="cpu", film=films[r]).init(5)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "film" in str(e) and "disagree" in str(e) for e in errs), errs


def test_option_and_refusals(gol, monkeypatch):
    monkeypatch.delenv("GOL_FILM", raising=False)
    plain = gol.Simulation(16, backend="cpu").init(5)
    assert plain.stats()["film"] is None and plain.config.film is None
    for call in (plain.film, plain.film_clear):
        with pytest.raises(ValueError) as e:
            call()
        assert "film=" in str(e.value)
    with pytest.raises(gol.native.GolError) as e:  # the engine on its own
        plain.engine.film()
    assert "film mode" in str(e.value)
    monkeypatch.setenv("GOL_FILM", "3,-2,4,5")  # read per call
    assert gol.Simulation(16, backend="cpu").stats()["film"] == (3, -2, 4, 5)
    monkeypatch.setenv("GOL_FILM", "3,2,4")
    with pytest.raises(ValueError):
        gol.Simulation(16, backend="cpu")
    monkeypatch.delenv("GOL_FILM")
    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"compat": True}, "compat"),
                     ({"subtiles": 2}, "subtiles=2")]:
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="cpu", film=(0, 0, 8, 8), **kw)
        assert word in str(e.value) and "film" in str(e.value)
    for rect, boundary, word in [((0, 0, 65, 8), "torus", "1..64"), ((0, 0, 8, 65), "torus", "1..64"),
                                 ((0, 0, 0, 8), "torus", "1..64"), ((60, 0, 8, 8), "dead", "inside the bounded 64 x 64"),
                                 ((0, -1, 8, 8), "dead", "inside the bounded 64 x 64")]:
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="cpu", film=rect, boundary=boundary)
        assert word in str(e.value) and "film" in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:  # more than 2^22 cells
        gol.Simulation(4096, backend="cpu", film=(0, 0, 2049, 2048))
    assert "2^22" in str(e.value) and "window()" in str(e.value)
    gol.Simulation(4096, backend="cpu", film=(0, 0, 2048, 2048))  # (2^22 cells are taken)


def test_engine_refusals(gol):
    """The engine on its own: the same refusals from EngineConfig, naming the rectangle and the board."""
    dec = gol.native.make_decomposition(64, 1, False, "1d", "", 0)
    geo = gol.native.make_geometry(dec, 0)

    def create(film, **kw):
        cfg = gol.native.EngineConfig()
        cfg.backend = "cpu"
        cfg.film = film
        for k, v in kw.items():
            setattr(cfg, k, v)
        return gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())

    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"compat": True}, "GOL_COMPAT"),
                     ({"subtiles": 2}, "GOL_SUBTILES=2")]:
        with pytest.raises(gol.native.GolError) as e:
            create((0, 0, 8, 8), **kw)
        assert word in str(e.value) and "film" in str(e.value)
    with pytest.raises(gol.native.GolError) as e:
        create((0, 0, 65, 8))
    assert "65 x 8" in str(e.value) and "1..64" in str(e.value)
    with pytest.raises(gol.native.GolError) as e:
        create((60, 3, 8, 8), boundary="dead")
    assert "8 x 8 cells at (60, 3)" in str(e.value) and "64 x 64" in str(e.value)
    with pytest.raises(ValueError):
        create((1, 2, 3))
    create((60, 3, 8, 8))  # (the torus wraps)


# ----- the CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_BOUNDARY",
              "GOL_PATTERN_FILE", "GOL_PATTERN_AT", "GOL_RLE_OUT", "GOL_CENSUS", "GOL_CENSUS_OUT", "GOL_COMPAT", "GOL_SUBTILES",
              "GOL_SIGNATURE", "GOL_SIGNATURE_OUT", "GOL_FILM", "GOL_FILM_OUT"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("boundary", fc.BOUNDARIES)
def test_cli_film_out(gol_bin, tmp_path, P, boundary):
    N, gens, rule = 48, 13, "B36/S23"
    H = N * P
    rect = (H - 5, 40, 12, 20) if boundary == "torus" else (H - 12, 20, 12, 20)
    r = _cli(gol_bin, [5, N, gens, 64, 0], tmp_path, GOL_FILM=",".join(map(str, rect)), GOL_FILM_OUT=tmp_path / "film.npy",
             GOL_NRANKS=P, GOL_RULE=rule, GOL_BOUNDARY=boundary, GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    raw = (tmp_path / "film.npy").read_bytes()
    assert raw[:8] == b"\x93NUMPY\x01\x00" and (10 + int.from_bytes(raw[8:10], "little")) % 64 == 0
    got = np.load(tmp_path / "film.npy")
    ref = numpy_film(initial_board(5, N, P, True), rule, gens, rect, bounded=boundary == "dead")
    assert got.dtype == np.uint8 and got.shape == (gens, 12, 20)
    assert np.array_equal(got, ref) and len({f.tobytes() for f in ref}) >= 2
    assert json.loads((tmp_path / "m.json").read_text())["film"] == list(rect)


def test_cli_film_flag_alone_and_default(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "a", GOL_FILM="1,2,3,4", GOL_METRICS_JSON=tmp_path / "a" / "m.json")
    assert r.returncode == 0, r.stderr
    assert json.loads((tmp_path / "a" / "m.json").read_text())["film"] == [1, 2, 3, 4]
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "b", GOL_METRICS_JSON=tmp_path / "b" / "m.json")
    assert r.returncode == 0, r.stderr
    assert json.loads((tmp_path / "b" / "m.json").read_text())["film"] is None


@pytest.mark.parametrize("P", [1, 3])
def test_cli_unwritable_path(gol_bin, tmp_path, P):
    bad = tmp_path / "no" / "such" / "dir" / "film.npy"
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_FILM="0,0,8,8", GOL_FILM_OUT=bad, GOL_NRANKS=P)
    assert r.returncode != 0 and str(bad) in r.stderr and "GOL_FILM_OUT" in r.stderr


def test_cli_film_out_needs_film(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_FILM_OUT=tmp_path / "film.npy")
    assert r.returncode != 0 and "GOL_FILM_OUT needs GOL_FILM" in r.stderr
    assert not (tmp_path / "film.npy").exists()


@pytest.mark.parametrize("env,word", [({"GOL_COMPAT": "reference"}, "film"), ({"GOL_SUBTILES": 2}, "film"),
                                      ({"GOL_CENSUS": 1}, "film"), ({"GOL_SIGNATURE": 1}, "film"),
                                      ({"GOL_FILM": "0,0,49,8"}, "1..48"), ({"GOL_FILM": "0,0,8"}, "r0,c0,rows,cols"),
                                      ({"GOL_FILM": "44,0,8,8", "GOL_BOUNDARY": "dead"}, "bounded 48 x 48")],
                         ids=["compat", "subtiles", "census", "signature", "too_large", "malformed", "outside"])
def test_cli_refusals(gol_bin, tmp_path, env, word):
    env = {"GOL_FILM": "0,0,8,8", **env}
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, **env)
    assert r.returncode != 0 and word in r.stderr, r.stderr


def test_cli_film_out_too_many_bytes(gol_bin, tmp_path):
    """More than 2^30 bytes of frames is refused before the run; the message names the three factors."""
    r = _cli(gol_bin, [5, 2048, 300, 64, 0], tmp_path, GOL_FILM="0,0,2048,2048", GOL_FILM_OUT=tmp_path / "film.npy")
    assert r.returncode != 0 and "2^30" in r.stderr
    assert "300 iterations" in r.stderr and "2048 rows" in r.stderr and "2048 columns" in r.stderr
