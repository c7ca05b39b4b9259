"""Density-film mode on the CPU backend, the oracle and the CLI: per-generation density maps of the whole board
(``density_film=(block_rows, block_cols)``, ``Simulation.density_film()``) against ``numpy_density_film``; the depth and
size sweep up to 200 cells a side, the block shapes, the start / clear / restart rules, thread ranks in 1-D and 2-D
grids, ranks that disagree, ``numpy_density_film`` against a literal per-cell count, ``GOL_DENSITY_FILM_OUT`` and the
refusals."""
import json
import threading

import numpy as np
import pytest

import density_film_cases as dc
import wide_cases as wc
from gol_amd.ops import initial_board, numpy_density_film, numpy_step_rule, numpy_step_rule_bounded, random_board


def _sim(gol, N, **kw):
    kw.setdefault("backend", "cpu")
    return gol.Simulation(N, **kw)


@pytest.mark.parametrize("N", [n for n in dc.SIZES if n <= 200])
@pytest.mark.parametrize("K", dc.DEPTHS)
def test_sweep(gol, K, N):
    dc.run_sweep_case(lambda n, **kw: _sim(gol, n, **kw), K, N, kernel="cpu")


@pytest.mark.parametrize("K", [8, 3])
@pytest.mark.parametrize("blocks", dc.SHAPE_BLOCKS, ids=lambda b: f"{b[0]}x{b[1]}")
def test_block_shapes(gol, blocks, K):
    dc.run_shape_case(lambda n, **kw: _sim(gol, n, **kw), blocks, K)


def test_numpy_density_film_against_a_per_cell_count():
    """The oracle itself, cell by cell on a 7 x 130 board: both boundaries, partial last blocks in both directions, one
    int for square blocks."""
    H, W, gens, rule = 7, 130, 5, "B36/S23"
    for bounded in (False, True):
        for blocks in ((3, 64), 64, (7, 192)):
            br, bc = (blocks, blocks) if isinstance(blocks, int) else blocks
            b = random_board(H, W, 4).astype(np.uint8)
            got, last = numpy_density_film(b, rule, gens, blocks, bounded=bounded, return_board=True)
            assert got.shape == (gens, -(-H // br), -(-W // bc)) and got.dtype == np.uint32
            for g in range(gens):
                b = (numpy_step_rule_bounded if bounded else numpy_step_rule)(b, rule, 1)
                want = np.zeros(got.shape[1:], np.uint32)
                for y in range(H):
                    for x in range(W):
                        want[y // br, x // bc] += int(b[y, x])
                assert np.array_equal(got[g], want), (bounded, blocks, g)
            assert np.array_equal(last, b) and len({m.tobytes() for m in got}) >= 2


def test_one_block_is_the_census(gol):
    N, gens, rule = 137, 17, dc.HIGHLIFE
    a = _sim(gol, N, rule=rule, halo_depth=8, density_film=(N, 192)).init(5, seed=3)
    b = _sim(gol, N, rule=rule, halo_depth=8, census=True).init(5, seed=3)
    a.step(gens)
    b.step(gens)
    start, maps = a.density_film()
    assert start == 0 and maps.shape == (gens, 1, 1)
    assert np.array_equal(maps[:, 0, 0].astype(np.uint64), b.census()[1]) and len(set(maps[:, 0, 0].tolist())) >= 2


@pytest.mark.parametrize("boundary", dc.BOUNDARIES)
def test_same_maps_as_step_density_loop(gol, boundary):
    N, gens, rule, blocks = 200, 21, dc.HIGHLIFE, (7, 64)
    a = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=8, density_film=blocks).init(5, seed=4)
    b = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=8).init(5, seed=4)
    a.step(gens)
    loop = []
    for _ in range(gens):
        b.step(1)
        loop.append(b.density(*blocks))
    start, got = a.density_film()
    assert start == 0 and np.array_equal(got, np.stack(loop)) and len({m.tobytes() for m in got}) >= 2
    assert np.array_equal(a.board(), b.board())


def test_start_clear_restart_rules(gol, tmp_path):
    """Several step() calls around a stamp(), set_board(), density_film_clear(), checkpoint() / restore() and init()."""
    N, rule, blocks, seed = 137, dc.HIGHLIFE, (7, 64), 8
    s = _sim(gol, N, rule=rule, halo_depth=8, density_film=blocks).init(5, seed=seed)
    assert s.density_film()[0] == 0 and s.density_film()[1].shape == (0, 20, 3)
    ref = dc.maps_of(N, N, seed, rule, "torus", 29, blocks)
    boards = dc.boards_of(N, N, seed, rule, "torus", 29)
    s.step(5).step(20).step(1)
    dc.check(s, 0, ref[:26], boards[:26], blocks)
    s.density_film_clear()
    assert s.density_film()[0] == 26 and len(s.density_film()[1]) == 0
    s.step(3)
    dc.check(s, 26, ref[26:], boards[26:], blocks)
    # stamp() and set_board() leave the record running
    s.stamp(np.ones((3, 3), np.uint8), at=(110, 130), mode="xor")
    b = s.board()
    s.set_board(b)
    s.step(4)
    start, got = s.density_film()
    assert start == 26 and len(got) == 7 and np.array_equal(got[:3], ref[26:])
    after, b4 = numpy_density_film(b, rule, 4, blocks, return_board=True)
    assert np.array_equal(got[3:], after)
    # checkpoint / restore: the record restarts at the restored generation
    s.checkpoint(str(tmp_path / "ck"))
    s.step(2)
    assert s.restore(str(tmp_path / "ck")) == 33
    assert s.density_film()[0] == 33 and len(s.density_film()[1]) == 0
    s.step(5)
    start, got = s.density_film()
    assert start == 33 and np.array_equal(got, numpy_density_film(b4, rule, 5, blocks))
    # init() starts it at 0
    s.init(5, seed=seed)
    s.step(7)
    dc.check(s, 0, ref[:7], boards[:7], blocks)


@pytest.mark.parametrize("boundary", dc.BOUNDARIES)
@pytest.mark.parametrize("name", ["1d3", "1d4", "2x2", "3x3"])
def test_thread_ranks(gol, name, boundary):
    P, kw, H, W, _ = dc.RANK_CASES[name]
    for blocks in dc.RANK_BLOCKS:
        ref, boards = dc.rank_ref(name, dc.HIGHLIFE, boundary, blocks)
        assert dc.distinct(H, W, dc.RANK_SEED, dc.HIGHLIFE, boundary, dc.RANK_GENS, blocks)
        assert boundary == "torus" or dc.told_apart(H, W, dc.RANK_SEED, dc.HIGHLIFE, dc.RANK_GENS, blocks)
        parts = wc.run_ranks(gol, P, H, W, "cpu", script=dc.film_script, rule=dc.HIGHLIFE, boundary=boundary, density_film=blocks, **kw)
        assert np.array_equal(wc.assemble(H, W, parts), boards[-1])
        dc.check_rank_parts(parts, ref, boards, blocks)


@pytest.mark.parametrize("films", [[(8, 64), None, (8, 64)], [(8, 64), (9, 64), (8, 64)], [(8, 64), (8, 128), (8, 64)]],
                         ids=["mode", "rows", "cols"])
def test_ranks_disagree(gol, films):
    """Every rank raises at init and none hangs."""
    P = 3
    ts = gol.parallel.thread_transports(P)
    errs = [None] * P

    def rank_main(r):
        try:
            gol.Simulation(32, ts[r], backend="cpu", density_film=films[r]).init(5)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "density-film" in str(e) and "disagree" in str(e) for e in errs), errs


def test_option_and_refusals(gol, monkeypatch):
    monkeypatch.delenv("GOL_DENSITY_FILM", raising=False)
    plain = gol.Simulation(16, backend="cpu").init(5)
    assert plain.stats()["density_film"] is None and plain.config.density_film is None
    for call in (plain.density_film, plain.density_film_clear):
        with pytest.raises(ValueError) as e:
            call()
        assert "density_film=" in str(e.value)
    with pytest.raises(gol.native.GolError) as e:  # the engine on its own
        plain.engine.density_film()
    assert "density-film mode" in str(e.value)
    assert gol.native.max_density_depth() >= 1
    monkeypatch.setenv("GOL_DENSITY_FILM", "3,128")  # read per call
    assert gol.Simulation(16, backend="cpu").stats()["density_film"] == (3, 128)
    monkeypatch.setenv("GOL_DENSITY_FILM", "64")
    assert gol.Simulation(16, backend="cpu").stats()["density_film"] == (64, 64)
    for bad in ("3,2,4", "x", "3,"):
        monkeypatch.setenv("GOL_DENSITY_FILM", bad)
        with pytest.raises(ValueError) as e:
            gol.Simulation(16, backend="cpu")
        assert "GOL_DENSITY_FILM" in str(e.value)
    monkeypatch.delenv("GOL_DENSITY_FILM")
    assert gol.Simulation(16, backend="cpu", density_film=64).config.density_film == (64, 64)  # one int: square blocks
    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"film": (0, 0, 8, 8)}, "film"),
                     ({"compat": True}, "compat"), ({"subtiles": 2}, "subtiles=2")]:
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="cpu", density_film=(8, 64), **kw)
        assert word in str(e.value) and "density_film" in str(e.value)
    for blocks, N, word in [((0, 64), 64, "block_rows must be >= 1 (got 0)"), ((-2, 64), 64, "(got -2)"),
                            ((8, 65), 64, "multiple of 64"), ((8, 65), 64, "(got 65)"), ((8, 0), 64, "(got 0)"),
                            ((1, 64), 8256, "2^20"), ((1, 64), 8256, "8256 x 129 blocks"), ((8, 64, 1), 64, "block_rows, block_cols")]:
        with pytest.raises(ValueError) as e:
            gol.Simulation(N, backend="cpu", density_film=blocks)
        assert word in str(e.value) and "density_film" in str(e.value), str(e.value)
    gol.Simulation(8192, backend="cpu", density_film=(1, 64))  # (2^20 blocks are taken)
    # a block of 2^32 cells: its count would not fit (refused before any engine is created)
    for blocks in [(65536, 65536), (70000, 131072)]:
        with pytest.raises(ValueError) as e:
            gol.Simulation(65536, backend="cpu", density_film=blocks)
        assert "2^32" in str(e.value) and f"{blocks[0]} x {blocks[1]}" in str(e.value) and "density_film" in str(e.value), str(e.value)


def test_engine_refusals(gol):
    """The engine on its own: the same refusals from EngineConfig, each naming the offending value."""
    dec = gol.native.make_decomposition(64, 1, False, "1d", "", 0)
    geo = gol.native.make_geometry(dec, 0)

    def create(blocks, geo=geo, **kw):
        cfg = gol.native.EngineConfig()
        cfg.backend = "cpu"
        cfg.density_film = blocks
        for k, v in kw.items():
            setattr(cfg, k, v)
        return gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())

    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"film": (0, 0, 8, 8)}, "film"),
                     ({"compat": True}, "GOL_COMPAT"), ({"subtiles": 2}, "GOL_SUBTILES=2")]:
        with pytest.raises(gol.native.GolError) as e:
            create((8, 64), **kw)
        assert word in str(e.value) and "density" in str(e.value)
    for blocks, word in [((0, 64), "block_rows must be >= 1 (got 0)"), ((8, 100), "multiple of 64"), ((8, 100), "(got 100)")]:
        with pytest.raises(gol.native.GolError) as e:
            create(blocks)
        assert word in str(e.value), str(e.value)
    big = gol.native.make_geometry(gol.native.make_decomposition(8256, 1, False, "1d", "", 0), 0)
    with pytest.raises(gol.native.GolError) as e:
        create((1, 64), geo=big)
    assert "2^20" in str(e.value) and "8256 x 129" in str(e.value)
    huge = gol.native.make_geometry(gol.native.make_decomposition(65536, 1, False, "1d", "", 0), 0)
    with pytest.raises(gol.native.GolError) as e:  # a block of 2^32 cells (refused before the boards are allocated)
        create((65536, 65536), geo=huge)
    assert "2^32" in str(e.value) and "65536 x 65536 cells" in str(e.value) and "density_film" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        create((1, 2, 3))
    assert create((200, 640)).stats()["density_film"] == (200, 640)  # (blocks larger than the board: one block)


# ----- the CLI -----

@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("boundary", dc.BOUNDARIES)
def test_cli_density_film_out(gol_bin, tmp_path, P, boundary):
    N, gens, rule, blocks = 137, 13, "B36/S23", (7, 64)
    out = tmp_path / "maps.npy"
    r = dc.cli(gol_bin, [5, N, gens, 64, 0], tmp_path, GOL_DENSITY_FILM="7,64", GOL_DENSITY_FILM_OUT=out, GOL_NRANKS=P,
               GOL_RULE=rule, GOL_BOUNDARY=boundary, GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    assert raw[:8] == b"\x93NUMPY\x01\x00" and (10 + int.from_bytes(raw[8:10], "little")) % 64 == 0
    got = np.load(out)
    ref = numpy_density_film(initial_board(5, N, P, True), rule, gens, blocks, bounded=boundary == "dead")
    assert got.dtype == np.dtype("<u4") and got.shape == ref.shape == (gens, -(-N * P // 7), 3)
    assert np.array_equal(got, ref) and len({m.tobytes() for m in ref}) >= 2
    assert json.loads((tmp_path / "m.json").read_text())["density_film"] == [7, 64]


def test_cli_flag_alone_and_default(gol_bin, tmp_path):
    r = dc.cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "a", GOL_DENSITY_FILM="5,128", GOL_METRICS_JSON=tmp_path / "a" / "m.json")
    assert r.returncode == 0, r.stderr
    assert json.loads((tmp_path / "a" / "m.json").read_text())["density_film"] == [5, 128]
    r = dc.cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "b", GOL_DENSITY_FILM="64", GOL_METRICS_JSON=tmp_path / "b" / "m.json")
    assert r.returncode == 0, r.stderr
    assert json.loads((tmp_path / "b" / "m.json").read_text())["density_film"] == [64, 64]
    r = dc.cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "c", GOL_METRICS_JSON=tmp_path / "c" / "m.json")
    assert r.returncode == 0, r.stderr
    assert json.loads((tmp_path / "c" / "m.json").read_text())["density_film"] is None


@pytest.mark.parametrize("P", [1, 3])
def test_cli_unwritable_path(gol_bin, tmp_path, P):
    bad = tmp_path / "no" / "such" / "dir" / "maps.npy"
    r = dc.cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_DENSITY_FILM="8,64", GOL_DENSITY_FILM_OUT=bad, GOL_NRANKS=P)
    assert r.returncode != 0 and str(bad) in r.stderr and "GOL_DENSITY_FILM_OUT" in r.stderr


def test_cli_out_needs_the_mode(gol_bin, tmp_path):
    r = dc.cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_DENSITY_FILM_OUT=tmp_path / "maps.npy")
    assert r.returncode != 0 and "GOL_DENSITY_FILM_OUT needs GOL_DENSITY_FILM" in r.stderr
    assert not (tmp_path / "maps.npy").exists()


@pytest.mark.parametrize("env,word", [({"GOL_COMPAT": "reference"}, "density_film"), ({"GOL_SUBTILES": 2}, "density"),
                                      ({"GOL_CENSUS": 1}, "density_film"), ({"GOL_SIGNATURE": 1}, "density_film"),
                                      ({"GOL_FILM": "0,0,8,8"}, "density_film"),
                                      ({"GOL_DENSITY_FILM": "8,65"}, "(got 65)"), ({"GOL_DENSITY_FILM": "0,64"}, "(got 0)"),
                                      ({"GOL_DENSITY_FILM": "8,64,2"}, "block_rows[,block_cols]")],
                         ids=["compat", "subtiles", "census", "signature", "film", "cols", "rows", "malformed"])
def test_cli_refusals(gol_bin, tmp_path, env, word):
    env = {"GOL_DENSITY_FILM": "8,64", **env}
    r = dc.cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, **env)
    assert r.returncode != 0 and word in r.stderr, r.stderr


def test_cli_block_too_large(gol_bin, tmp_path):
    """A block of 2^32 cells is refused when the engine is made, before any board is allocated; the message names it."""
    r = dc.cli(gol_bin, [5, 65536, 1, 64, 0], tmp_path, GOL_DENSITY_FILM="65536")
    assert r.returncode != 0 and "2^32" in r.stderr and "65536 x 65536 cells" in r.stderr, r.stderr


def test_cli_out_too_many_bytes(gol_bin, tmp_path):
    """More than 2^30 bytes of maps is refused before the run; the message names the three factors."""
    r = dc.cli(gol_bin, [5, 8192, 300, 64, 0], tmp_path, GOL_DENSITY_FILM="1,64", GOL_DENSITY_FILM_OUT=tmp_path / "maps.npy")
    assert r.returncode != 0 and "2^30" in r.stderr
    assert "300 iterations" in r.stderr and "8192 x 128 blocks" in r.stderr
