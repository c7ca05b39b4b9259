"""Census mode (``census=True``: the global population of every generation a run computes) on the CPU backend, the
CLI and the Python API, against the numpy oracle ``numpy_census``.

Every comparison is exact, and each also asserts that the final board is the oracle's (counting must not disturb
stepping), that the last count is ``population()`` and that the series holds at least two distinct values.  Random
boards keep the ghost rows and words live, so a count that included a ghost cell would be wrong."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_census, numpy_step_rule, numpy_step_rule_bounded, random_board

RULES = ["B3/S23", "B36/S23", "B1357/S1357", "B1/S012345678"]
BOUNDARIES = ["torus", "dead"]
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8]
GLIDER = "x = 3, y = 3\nbob$2bo$3o!\n"


@functools.lru_cache(maxsize=None)
def sweep_reference(N, rule, boundary):
    """The oracle's series of the sweep's N x N board (seed N) over the longest run, 17 generations, and the boards
    after every odd generation: computed once per (N, rule, boundary) and shared by the depths."""
    b = initial_board(5, N, 1, True, N)
    counts, boards = [], {}
    for g in range(1, 2 * max(DEPTHS) + 2):
        b = (numpy_step_rule_bounded if boundary == "dead" else numpy_step_rule)(b, rule, 1)
        counts.append(int(b.sum()))
        if g % 2:
            boards[g] = b
    return np.array(counts, np.uint64), boards


def check(sim, start, counts, board, tiny=False):
    got_start, got = sim.census()
    assert got_start == start and got.dtype == np.uint64
    assert np.array_equal(got, counts), (got.tolist(), np.asarray(counts).tolist())
    assert np.array_equal(sim.board(), board)
    assert int(got[-1]) == sim.population()
    assert tiny or len(set(got.tolist())) >= 2


def test_numpy_census_is_a_per_generation_loop():
    for bounded, step in [(False, numpy_step_rule), (True, numpy_step_rule_bounded)]:
        b = random_board(37, 70, 3)
        want = []
        for g in range(1, 10):
            want.append(int(step(b, "B36/S23", g).sum()))
        got = numpy_census(b, "B36/S23", 9, bounded=bounded)
        assert got.dtype == np.uint64 and got.tolist() == want and len(set(want)) > 2
        counts, last = numpy_census(b, "B36/S23", 9, bounded=bounded, return_board=True)
        assert np.array_equal(counts, got) and np.array_equal(last, step(b, "B36/S23", 9))
    assert numpy_census(np.ones((3, 3), np.uint8), "B3/S23", 2, bounded=True).tolist() == [4, 0]
    assert numpy_census(np.ones((3, 3), np.uint8), "B3/S23", 2).tolist() == [0, 0]
    assert len(numpy_census(np.ones((3, 3), np.uint8), "B3/S23", 0)) == 0


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000])
@pytest.mark.parametrize("K", DEPTHS)
def test_sweep(gol, K, N):
    """Every superstep depth on every size class: a full superstep and the remainders (2K + 1 generations)."""
    gens = 2 * K + 1
    for boundary in BOUNDARIES:
        for rule in RULES:
            counts, boards = sweep_reference(N, rule, boundary)
            s = gol.Simulation(N, backend="cpu", rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, census=True)
            s.init(5, seed=N).step(gens)
            assert s.stats()["census"] is True
            check(s, 0, counts[:gens], boards[gens], tiny=N <= 3)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("H,W", [(70, 130), (100, 200), (200, 64), (5, 1000)])
def test_rectangular(gol, H, W, boundary):
    gens = 17
    counts, board = numpy_census(random_board(H, W, 5), "B36/S23", gens, bounded=boundary == "dead", return_board=True)
    s = gol.Simulation(H, backend="cpu", rule="B36/S23", boundary=boundary, width=W, halo_depth=8, census=True).init(5, seed=5)
    s.step(gens)
    check(s, 0, counts, board)


def test_several_steps_stamp_init_restore(gol, tmp_path):
    """One continuous series over several step() calls and a stamp(); init() and restore() clear it and set start."""
    N, rule = 70, "B36/S23"
    s = gol.Simulation(N, backend="cpu", rule=rule, halo_depth=4, census=True).init(5, seed=8)
    assert s.census()[0] == 0 and len(s.census()[1]) == 0
    b = initial_board(5, N, 1, True, 8)
    s.step(5).step(20).step(1)
    c1, b = numpy_census(b, rule, 26, return_board=True)
    check(s, 0, c1, b)
    s.stamp(GLIDER, at=(3, 3), mode="xor")  # the generation count runs on: so does the series
    b = s.board()
    s.step(7)
    c2, b = numpy_census(b, rule, 7, return_board=True)
    check(s, 0, np.concatenate([c1, c2]), b)
    s.checkpoint(str(tmp_path / "c"))
    s.census_clear()
    assert s.census()[0] == 33 and len(s.census()[1]) == 0
    s.step(3)
    c3, b3 = numpy_census(b, rule, 3, return_board=True)
    check(s, 33, c3, b3)
    s.init(5, seed=8)
    assert s.census()[0] == 0 and len(s.census()[1]) == 0
    s.step(2)
    assert np.array_equal(s.census()[1], c1[:2])
    assert s.restore(str(tmp_path / "c")) == 33
    assert s.census()[0] == 33 and len(s.census()[1]) == 0
    s.step(3)
    check(s, 33, c3, b3)
    s.load_rle(GLIDER)
    assert s.census()[0] == 0 and len(s.census()[1]) == 0
    s.step(4)
    assert s.census()[1].tolist() == [5, 5, 5, 5]


def _run_threads(gol, N, P, gens, backend="cpu", **kw):
    ts = gol.parallel.thread_transports(P)
    out, errs = [None] * P, []

    def worker(r):
        try:
            s = gol.Simulation(N, ts[r], backend=backend, global_mode=True, census=True, **kw).init(5, seed=99)
            s.step(gens)
            start, counts = s.census()
            out[r] = (s.geometry.row0, s.geometry.col0, s.board(), start, counts, s.population())
        except Exception as e:  # reported below
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    full = np.zeros((N, N), np.uint8)
    for r0, c0, b, *_ in out:
        full[r0 : r0 + b.shape[0], c0 : c0 + b.shape[1]] = b
    return full, out


@pytest.mark.parametrize("P,kw", [(3, {}), (4, {"decomp": "2d", "grid": "2x2"})], ids=["P3", "2x2"])
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_thread_ranks(gol, P, kw, boundary):
    """Every rank gets the same, global series; no rank counts a ghost cell of its neighbour's."""
    N, gens = 192, 19
    for rule in ("B36/S23", "B1/S012345678"):
        full, out = _run_threads(gol, N, P, gens, rule=rule, boundary=boundary, halo_depth=4, **kw)
        counts, board = numpy_census(initial_board(5, N, 1, True, 99), rule, gens, bounded=boundary == "dead", return_board=True)
        assert np.array_equal(full, board)
        for _, _, _, start, got, pop in out:
            assert start == 0 and np.array_equal(got, counts) and pop == int(counts[-1])
        assert len(set(counts.tolist())) >= 2


def test_rank_census_mismatch_raises_everywhere(gol):
    """Ranks that disagree on the census mode all raise at init, naming it; none hangs in census()."""
    P = 2
    ts = gol.parallel.thread_transports(P)
    errs = [None] * P

    def worker(r):
        try:
            gol.Simulation(64, ts[r], backend="cpu", census=bool(r)).init(5, seed=1)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "census" in str(e) and "disagree" in str(e) for e in errs), errs


def test_option_and_refusals(gol, monkeypatch):
    monkeypatch.delenv("GOL_CENSUS", raising=False)
    plain = gol.Simulation(16, backend="cpu").init(5)
    assert plain.stats()["census"] is False and plain.config.census is False
    with pytest.raises(ValueError) as e:
        plain.census()
    assert "census=True" in str(e.value)
    with pytest.raises(ValueError):
        plain.census_clear()
    with pytest.raises(gol.native.GolError) as e:  # the engine on its own
        plain.engine.census()
    assert "census mode" in str(e.value)
    monkeypatch.setenv("GOL_CENSUS", "1")
    assert gol.Simulation(16, backend="cpu").stats()["census"] is True
    assert gol.Simulation(16, backend="cpu", census=False).stats()["census"] is False
    monkeypatch.delenv("GOL_CENSUS")
    with pytest.raises(ValueError) as e:
        gol.Simulation(64, backend="cpu", census=True, compat=True)
    assert "compat" in str(e.value)
    with pytest.raises(ValueError) as e:
        gol.Simulation(64, backend="cpu", census=True, subtiles=2)
    assert "subtiles=2" in str(e.value)
    # the specialised HIP kernels and a pass deeper than the census kernel's (refused before any device is looked for)
    for kernel in ("temporal", "tile", "pipe", "resident", "lds"):
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="hip", census=True, kernel=kernel)
        assert f"kernel {kernel!r} counts no census" in str(e.value)
    D = gol.native.max_census_depth()
    assert D >= 4
    with pytest.raises(ValueError) as e:
        gol.Simulation(64, backend="hip", census=True, kernel_depth=D + 1)
    assert f"deepest pass, {D} generations" in str(e.value)
    # the native engine refuses compat and sub-tiles on its own as well
    sim = gol.Simulation(64, backend="cpu")
    for field, value in [("compat", True), ("subtiles", 2)]:
        cfg = gol.native.EngineConfig()
        cfg.census = True
        setattr(cfg, field, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(sim.geometry, cfg, sim.transport)
        assert "census" in str(e.value)


# ----- CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_BOUNDARY",
              "GOL_PATTERN_FILE", "GOL_PATTERN_AT", "GOL_RLE_OUT", "GOL_CENSUS", "GOL_CENSUS_OUT", "GOL_COMPAT", "GOL_SUBTILES"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


def _read_series(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "generation,population"
    rows = [tuple(int(v) for v in ln.split(",")) for ln in lines[1:]]
    return [g for g, _ in rows], [p for _, p in rows]


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_cli_census_out(gol_bin, tmp_path, P, boundary):
    N, gens, rule = 48, 13, "B36/S23"
    r = _cli(gol_bin, [5, N, gens, 64, 0], tmp_path, GOL_CENSUS_OUT=tmp_path / "pop.csv", GOL_NRANKS=P, GOL_RULE=rule,
             GOL_BOUNDARY=boundary, GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    g, pop = _read_series(tmp_path / "pop.csv")
    want = numpy_census(initial_board(5, N, P, True), rule, gens, bounded=boundary == "dead")
    assert g == list(range(1, gens + 1)) and pop == want.tolist() and len(set(pop)) >= 2
    assert '"census": true' in (tmp_path / "m.json").read_text()


def test_cli_census_flag_alone_and_default(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "a", GOL_CENSUS=1, GOL_METRICS_JSON=tmp_path / "a" / "m.json")
    assert r.returncode == 0, r.stderr
    assert '"census": true' in (tmp_path / "a" / "m.json").read_text()
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "b", GOL_METRICS_JSON=tmp_path / "b" / "m.json")
    assert r.returncode == 0, r.stderr
    assert '"census": false' in (tmp_path / "b" / "m.json").read_text()


@pytest.mark.parametrize("P", [1, 3])
def test_cli_unwritable_path(gol_bin, tmp_path, P):
    bad = tmp_path / "no" / "such" / "dir" / "pop.csv"
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_CENSUS_OUT=bad, GOL_NRANKS=P)
    assert r.returncode != 0 and str(bad) in r.stderr and "GOL_CENSUS_OUT" in r.stderr


@pytest.mark.parametrize("env", [{"GOL_COMPAT": "reference"}, {"GOL_SUBTILES": 2}], ids=["compat", "subtiles"])
def test_cli_refusals(gol_bin, tmp_path, env):
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_CENSUS=1, **env)
    assert r.returncode != 0 and "census" in r.stderr
