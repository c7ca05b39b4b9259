"""Density-film mode on the HIP backend: the kernel step_density<K> (density_kernel.hip, nbhd_density_kernel.hip) under
every schedule the census kernel runs under -- pass depths, board sizes, wrap and ghost rows, both boundaries, block
shapes, wide boards with full-width segments, multi-pass supersteps, a map buffer forced small, thread ranks sharing the
GPU, rank grids, the 1-rank RCCL communicator, the other neighbourhoods, the CLI -- against the numpy oracle
``numpy_density_film``.

Every comparison is exact, and each also asserts the ``density@`` kernel, ``stats()["density_film"]``, that every map
sums to the population of the oracle's board and that the final board is the oracle's (density_film_cases.check).
Random boards keep the ghost rows and words live, so a map that counts a redundantly computed cell, or misses an owned
one, is wrong."""
import json

import numpy as np
import pytest

import density_film_cases as dc
import wide_cases as wc
from gol_amd.ops import initial_board, numpy_density_film, numpy_film, random_board

pytestmark = pytest.mark.gpu


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


def test_depths_are_instantiated(gol):
    assert gol.native.max_density_depth() == 8


@pytest.mark.parametrize("N", dc.SIZES)
@pytest.mark.parametrize("K", dc.DEPTHS)
def test_sweep(gol, K, N):
    """Every pass depth on every size class (wrap rows on boards shorter than the pass, where one owned row is computed
    many times and the row counter runs on while the load row wraps; tail words of 1, 63 and 9 cells; packed segments
    in the per-lane runner; several workgroups); the block shapes cycle with the case."""
    dc.run_sweep_case(lambda n, **kw: _sim(gol, n, **kw), K, N, kernel="density@")  # (a 1-, 2- or 3-row board clamps the depth)


@pytest.mark.parametrize("K", [8, 3])
@pytest.mark.parametrize("blocks", dc.SHAPE_BLOCKS, ids=lambda b: f"{b[0]}x{b[1]}")
def test_block_shapes(gol, blocks, K):
    dc.run_shape_case(lambda n, **kw: _sim(gol, n, **kw), blocks, K, kernel=f"density@{K}")


# (16, 128): many block ends inside every segment.  (9, 3968): 62-word block columns, the width of a full-width segment:
# on the 4096- and 8000-column boards the second block column holds the packed remainder (and, at 8000, the second
# full-width segment), so lanes of one wave add into one counter and waves of both runners into the same block.
WIDE = [(wc.S4096, 0), (wc.S3969, 0), (wc.S8000, 0), (wc.TALL, wc.TALL_ROWS)]
WIDE_BLOCKS = [(16, 128), (9, 3968)]


@pytest.mark.parametrize("shape,rows", WIDE, ids=[wc.shape_id(s) for s, _ in WIDE])
@pytest.mark.parametrize("K", [5, 8])
def test_wide(gol, K, shape, rows):
    """Full-width segments in the scalar runner (wide_cases.py tells what each shape gives)."""
    gens = 2 * K + 1
    H, W = shape.H, shape.W
    rule = dc.HIGHLIFE
    for boundary in dc.BOUNDARIES:
        board = wc.board_after(shape, rule, boundary, gens)
        pops = wc.counts_until(shape, rule, boundary, gens)
        for blocks in WIDE_BLOCKS:
            ref = dc.maps_of(H, W, wc.SEED, rule, boundary, wc.SWEEP_GENS, blocks)[:gens]
            assert len({m.tobytes() for m in ref}) >= 2
            assert boundary == "torus" or dc.told_apart(H, W, wc.SEED, rule, wc.SWEEP_GENS, blocks, upto=gens)
            assert np.array_equal(ref.reshape(gens, -1).sum(axis=1, dtype=np.uint64), pops)
            s = _sim(gol, H, width=W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, rows_per_wave=rows,
                     density_film=blocks).init(5, seed=wc.SEED)
            s.step(gens)
            st = s.stats()
            assert st["density_film"] == blocks and st["kernel"].startswith(f"density@{K}"), st
            start, got = s.density_film()
            assert start == 0 and got.dtype == np.uint32 and np.array_equal(got, ref)
            assert np.array_equal(s.board(), board)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("boundary", dc.BOUNDARIES)
@pytest.mark.parametrize("passes", [2, 3])
def test_multipass_supersteps(gol, passes, boundary, graph):
    """Supersteps of two and three passes of depth 8 plus a remainder: the extension rows the earlier passes compute
    beyond the tile are not counted; launches are eager whatever GOL_GRAPH says."""
    N, R, gens, seed, blocks = 137, 8 * passes, 37, 6, (7, 64)
    for rule in dc.RULES:
        assert dc.lively(N, N, seed, rule, boundary, gens, blocks)
        s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=R, kernel_depth=8, graph=bool(graph), density_film=blocks).init(5, seed=seed)
        st = s.stats()
        assert st["depth"] == R and st["kernel_depth"] == 8, st
        s.step(gens)
        assert s.stats()["graph_launches"] == 0
        dc.check(s, 0, dc.maps_of(N, N, seed, rule, boundary, gens, blocks), dc.boards_of(N, N, seed, rule, boundary, gens), blocks,
                 "density@8")


def test_several_steps_clear_init_restore(gol, tmp_path):
    """Several step() calls around a stamp(), density_film_clear(), checkpoint() / restore() and init(); start every time."""
    N, rule, blocks, seed = 137, dc.HIGHLIFE, (7, 64), 8
    s = _sim(gol, N, rule=rule, halo_depth=8, density_film=blocks).init(5, seed=seed)
    assert s.density_film()[0] == 0 and s.density_film()[1].shape == (0, 20, 3)  # (the init-time timing launches left nothing)
    ref = dc.maps_of(N, N, seed, rule, "torus", 29, blocks)
    boards = dc.boards_of(N, N, seed, rule, "torus", 29)
    s.step(5).step(20).step(1)
    dc.check(s, 0, ref[:26], boards[:26], blocks, "density@8")
    s.density_film_clear()
    assert s.density_film()[0] == 26 and len(s.density_film()[1]) == 0
    s.step(3)
    dc.check(s, 26, ref[26:], boards[26:], blocks)
    s.stamp(np.ones((3, 3), np.uint8), at=(110, 130), mode="xor")  # (leaves the record running)
    b = s.board()
    s.step(4)
    start, got = s.density_film()
    assert start == 26 and len(got) == 7 and np.array_equal(got[:3], ref[26:])
    after, b4 = numpy_density_film(b, rule, 4, blocks, return_board=True)
    assert np.array_equal(got[3:], after)
    s.checkpoint(str(tmp_path / "ck"))
    s.step(2)
    assert s.restore(str(tmp_path / "ck")) == 33
    assert s.density_film()[0] == 33 and len(s.density_film()[1]) == 0
    s.step(5)
    start, got = s.density_film()
    assert start == 33 and np.array_equal(got, numpy_density_film(b4, rule, 5, blocks))
    s.init(5, seed=seed)
    s.step(7)
    dc.check(s, 0, ref[:7], boards[:7], blocks)


def test_small_buffer_chunks(gol, monkeypatch):
    """GOL_DENSITY_FILM_MB=1: a map of the 1000 x 16 grid of (1, 64) blocks takes 64000 bytes, the buffer holds 16 of
    them, and 40 generations take three chunks.  A grid of which fewer than 8 maps fit is refused at init."""
    monkeypatch.setenv("GOL_DENSITY_FILM_MB", "1")
    N, gens, rule, blocks = 1000, 40, dc.HIGHLIFE, (1, 64)
    per_chunk = (1 << 20) // (1000 * 16 * 4)
    assert 8 <= per_chunk and -(-gens // per_chunk) >= 3
    s = _sim(gol, N, rule=rule, halo_depth=16, kernel_depth=8, density_film=blocks).init(5, seed=2)
    s.step(gens)
    start = random_board(N, N, 2)
    ref = numpy_density_film(start, rule, gens, blocks)
    boards = numpy_film(start, rule, gens, (0, 0, N, N))
    assert len({m.tobytes() for m in ref}) >= 2
    dc.check(s, 0, ref, boards, blocks, "density@8")
    with pytest.raises(gol.native.GolError) as e:  # 2048 x 32 blocks: 262144 bytes a map, four in 1 MiB
        _sim(gol, 2048, rule=rule, density_film=blocks)
    assert "GOL_DENSITY_FILM_MB" in str(e.value) and "2048 x 32 blocks" in str(e.value)
    monkeypatch.setenv("GOL_DENSITY_FILM_MB", "0")
    with pytest.raises(gol.native.GolError) as e:
        _sim(gol, 64, rule=rule, density_film=(8, 64))
    assert "GOL_DENSITY_FILM_MB must be in 1..2047 (got 0)" in str(e.value)


def test_one_block_is_the_census(gol):
    N, gens, rule = 1000, 19, dc.HIGHLIFE
    a = _sim(gol, N, rule=rule, halo_depth=8, density_film=(N, 1024)).init(5, seed=3)
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


@pytest.mark.parametrize("boundary", dc.BOUNDARIES)
@pytest.mark.parametrize("name,kw", [("1d3", {}), ("1d4", {"schedule": "split"}), ("1d4", {"schedule": "full"}), ("2x2", {}), ("3x3", {})],
                         ids=["P3", "P4-split", "P4-full", "2x2", "3x3"])
def test_thread_ranks(gol, name, kw, boundary):
    """Thread ranks on hip against numpy: strips under the split and the full schedule (the interior and the bands of
    a split pass add into the same counters from two streams), a 2 x 2 and a 3 x 3 grid; the blocks are
    density_film_cases.RANK_BLOCKS, with which ranks add into the same blocks.  Supersteps of two passes and remainders; every rank gets every map."""
    P, grid, H, W, _ = dc.RANK_CASES[name]
    rule = dc.HIGHLIFE
    for blocks in dc.RANK_BLOCKS:
        ref, boards = dc.rank_ref(name, rule, boundary, blocks)
        assert dc.distinct(H, W, dc.RANK_SEED, rule, boundary, dc.RANK_GENS, blocks)
        assert boundary == "torus" or dc.told_apart(H, W, dc.RANK_SEED, rule, dc.RANK_GENS, blocks)
        parts = wc.run_ranks(gol, P, H, W, "hip", script=dc.film_script, rule=rule, boundary=boundary, density_film=blocks,
                             **grid, **kw)
        assert np.array_equal(wc.assemble(H, W, parts), boards[-1])
        dc.check_rank_parts(parts, ref, boards, blocks)
        for p in parts:
            st = p.result[2]
            assert st["kernel"].startswith("density@"), st
            if "schedule" in kw:
                assert ("+boundary:density@" in st["kernel"]) == (kw["schedule"] == "split"), st


@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


def test_rccl_self(gol, rccl):
    N, R, gens, rule, boundary, blocks = 256, 16, 40, dc.HIGHLIFE, "torus", (7, 64)
    s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=rule, boundary=boundary, halo_depth=R,
                       kernel_depth=8, subtiles=0, density_film=blocks)
    s.init(5, seed=R)
    s.step(gens)
    st = s.stats()
    assert st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
    assert dc.lively(N, N, R, rule, boundary, gens, blocks)
    dc.check(s, 0, dc.maps_of(N, N, R, rule, boundary, gens, blocks), dc.boards_of(N, N, R, rule, boundary, gens), blocks, "density@8")
    s.synchronize()


@pytest.mark.parametrize("K", [8, 3])
@pytest.mark.parametrize("rule", ["B13/S13V", "B2/S34H"])
def test_neighbourhoods(gol, rule, K):
    dc.run_shape_case(lambda n, **kw: _sim(gol, n, **kw), (5, 64), K, kernel=f"density@{K}", rules=[rule], seed=12, gens=2 * K + 3)


def test_run_hint_prediction_leaves_no_map(gol):
    N, gens, rule, blocks = 200, 21, dc.HIGHLIFE, (8, 128)
    s = _sim(gol, N, rule=rule, halo_depth=8, run_hint=gens, density_film=blocks).init(5, seed=3)
    assert s.generation == 0 and len(s.density_film()[1]) == 0
    s.step(gens)
    dc.check(s, 0, dc.maps_of(N, N, 3, rule, "torus", gens, blocks), dc.boards_of(N, N, 3, rule, "torus", gens), blocks, "density@8")


def test_refusals(gol):
    ok = (8, 64)
    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"film": (0, 0, 8, 8)}, "film"),
                     ({"compat": True}, "compat"), ({"subtiles": 2}, "subtiles=2"), ({"kernel_depth": 9}, "kernel_depth 9")] + [
                         ({"kernel": k}, k) for k in ("temporal", "tile", "pipe", "resident", "lds")]:
        with pytest.raises(ValueError) as e:
            _sim(gol, 64, density_film=ok, **kw)
        assert word in str(e.value) and "density" in str(e.value), str(e.value)
    for blocks, N, word in [((0, 64), 64, "(got 0)"), ((8, 96), 64, "(got 96)"), ((1, 64), 8256, "8256 x 129 blocks"),
                            ((65536, 65536), 65536, "65536 x 65536 cells holds more than 2^32")]:
        with pytest.raises(ValueError) as e:
            _sim(gol, N, density_film=blocks)
        assert word in str(e.value), str(e.value)
    # the engine on its own refuses the same
    dec = gol.native.make_decomposition(64, 1, False, "1d", "", 0)
    geo = gol.native.make_geometry(dec, 0)
    for attr, value, word in [("kernel_depth", 9, "kernel_depth 9"), ("kernel", "temporal", "temporal"), ("kernel", "lds", "lds"),
                              ("census", True, "census"), ("signature", True, "signature"), ("film", (0, 0, 8, 8), "film"),
                              ("density_film", (8, 96), "(got 96)"), ("density_film", (0, 64), "(got 0)")]:
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.device = "hip", 0
        cfg.density_film = ok
        setattr(cfg, attr, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
        assert word in str(e.value), str(e.value)


@pytest.mark.parametrize("boundary", dc.BOUNDARIES)
def test_cli_density_film_out(gol_bin, tmp_path, boundary):
    N, gens, rule, blocks = 137, 13, "B36/S23", (7, 64)
    out = tmp_path / "maps.npy"
    r = dc.cli(gol_bin, [5, N, gens, 64, 0], tmp_path, backend="hip", GOL_DENSITY_FILM="7,64", GOL_DENSITY_FILM_OUT=out,
               GOL_RULE=rule, GOL_BOUNDARY=boundary, GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    got = np.load(out)
    ref = numpy_density_film(initial_board(5, N, 1, True), rule, gens, blocks, bounded=boundary == "dead")
    assert got.dtype == np.dtype("<u4") and got.shape == ref.shape == (gens, 20, 3)
    assert np.array_equal(got, ref) and len({m.tobytes() for m in ref}) >= 2
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["density_film"] == [7, 64] and m["kernel"].startswith("density@"), m
