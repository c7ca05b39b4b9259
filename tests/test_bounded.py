"""Bounded boards (``boundary="dead"``: every cell outside the board is dead in every generation) on the CPU
backend, the CLI and the Python API, against the zero-padded numpy oracle ``numpy_step_rule_bounded``.

Every comparison also asserts that the bounded result differs from the torus oracle's for its input, so a run
that ignored the boundary could not pass."""
import os
import subprocess
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_step_rule, numpy_step_rule_bounded, random_board
from gol_amd.utils import read_dump

RULES = ["B3/S23", "B36/S23", "B1357/S1357", "B1/S012345678"]
GLIDER = "x = 3, y = 3\nbob$2bo$3o!\n"


def oracle(board, rule, gens):
    """The bounded oracle's result, checked to differ from the torus oracle's on this input."""
    ref = numpy_step_rule_bounded(board, rule, gens)
    assert not np.array_equal(ref, numpy_step_rule(board, rule, gens)), "the input does not tell the boundaries apart"
    return ref


def test_oracle_by_hand():
    """The oracle itself on cases small enough to know: a full 3 x 3 board, and a blinker flat against an edge."""
    full = np.ones((3, 3), np.uint8)
    # corners have 3 neighbours (survive), edge cells 5 and the centre 8 (die)
    assert np.array_equal(numpy_step_rule_bounded(full, "B3/S23", 1), [[1, 0, 1], [0, 0, 0], [1, 0, 1]])
    assert np.array_equal(numpy_step_rule(full, "B3/S23", 1), np.zeros((3, 3)))  # (on the torus all have 8)
    b = np.zeros((4, 5), np.uint8)
    b[0, 1:4] = 1  # a horizontal blinker on the top row: the cell above its centre does not exist
    assert np.array_equal(numpy_step_rule_bounded(b, "B3/S23", 1), [[0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0] * 5, [0] * 5])
    one = np.ones((1, 1), np.uint8)
    assert numpy_step_rule_bounded(one, "B1/S012345678", 3)[0, 0] == 1 and numpy_step_rule_bounded(one, "B3/S23", 1)[0, 0] == 0


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sweep(gol, K, N):
    """Every superstep depth on every size class: a full superstep and the remainders (2K + 1 generations)."""
    gens = 2 * K + 1
    board = initial_board(5, N, 1, True, N + K)
    for rule in RULES:
        s = gol.Simulation(N, backend="cpu", rule=rule, boundary="dead", halo_depth=K, kernel_depth=K).init(5, seed=N + K)
        s.step(gens)
        ref = numpy_step_rule_bounded(board, rule, gens)
        assert np.array_equal(s.board(), ref), (rule, N, K)
        # (boards of 1 to 3 cells a side die out under either boundary, and B1/S012345678 fills both)
        if N >= 63 and rule != "B1/S012345678":
            assert not np.array_equal(ref, numpy_step_rule(board, rule, gens)), (rule, N, K)


@pytest.mark.parametrize("H,W", [(70, 130), (100, 200), (200, 64), (5, 1000)])
def test_rectangular(gol, H, W):
    gens = 17
    board = random_board(H, W, 5)
    s = gol.Simulation(H, backend="cpu", rule="B36/S23", boundary="dead", width=W, halo_depth=8).init(5, seed=5)
    s.step(gens)
    assert np.array_equal(s.board(), oracle(board, "B36/S23", gens))


def _run_threads(gol, N, P, gens, backend="cpu", transports=None, **kw):
    ts = transports if transports is not None else gol.parallel.thread_transports(P)
    boards, errs = [None] * P, []

    def worker(r):
        try:
            s = gol.Simulation(N, ts[r], backend=backend, **kw).init(5, seed=99)
            s.step(gens)
            boards[r] = (s.geometry.row0, s.geometry.col0, s.board())
        except Exception as e:  # reported below
            errs.append(e)

    th = [threading.Thread(target=worker, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    dec = gol.parallel.decomposition(N, P, kw.get("global_mode", False), kw.get("decomp", "1d"), kw.get("grid", ""), 0)
    full = np.zeros((dec.H, dec.W), np.uint8)
    for r0, c0, b in boards:
        full[r0 : r0 + b.shape[0], c0 : c0 + b.shape[1]] = b
    return full


@pytest.mark.parametrize("P,kw", [(2, {}), (4, {}), (4, {"decomp": "2d", "grid": "2x2", "global_mode": True})],
                         ids=["P2", "P4", "2x2"])
@pytest.mark.parametrize("rule", ["B36/S23", "B1/S012345678"])
def test_thread_ranks(gol, P, kw, rule):
    """The torus exchanges keep running; what they deliver across a global edge is masked away."""
    N, gens = (96, 19) if not kw else (192, 19)
    full = _run_threads(gol, N, P, gens, rule=rule, boundary="dead", halo_depth=4, **kw)
    per_rank = not kw.get("global_mode", False)
    board = initial_board(5, N, P, per_rank, 99)
    ref = numpy_step_rule_bounded(board, rule, gens)
    assert np.array_equal(full, ref)
    if rule == "B36/S23":
        assert not np.array_equal(ref, numpy_step_rule(board, rule, gens))


def test_rank_boundary_mismatch_raises_everywhere(gol):
    """Ranks that disagree on the boundary all raise at init, naming both; none hangs."""
    P = 2
    ts = gol.parallel.thread_transports(P)
    errs = [None] * P

    def worker(r):
        try:
            gol.Simulation(64, ts[r], backend="cpu", boundary=["dead", "torus"][r]).init(5, seed=1)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "boundary" in str(e) and "dead" in str(e) and "torus" in str(e) for e in errs), errs


# ----- the option through the layers -----

def test_default_is_the_torus(gol, monkeypatch):
    monkeypatch.delenv("GOL_BOUNDARY", raising=False)
    s = gol.Simulation(16, backend="cpu")
    assert s.stats()["boundary"] == "torus" and s.config.boundary == "torus" and "boundary" not in s.describe()
    d = gol.Simulation(16, backend="cpu", boundary="dead").init(5)
    assert d.stats()["boundary"] == "dead" and d.describe().endswith(", boundary dead")
    monkeypatch.setenv("GOL_BOUNDARY", "dead")
    assert gol.Simulation(16, backend="cpu").stats()["boundary"] == "dead"
    assert gol.Simulation(16, backend="cpu", boundary="torus").stats()["boundary"] == "torus"


@pytest.mark.parametrize("bad", ["banana", "", "Dead", "plane"])
def test_bad_boundary_is_a_value_error(gol, bad):
    with pytest.raises(ValueError) as e:
        gol.Simulation(16, backend="cpu", boundary=bad)
    assert f"'{bad}'" in str(e.value)


def test_refusals(gol):
    with pytest.raises(ValueError) as e:
        gol.Simulation(64, backend="cpu", boundary="dead", compat=True)
    assert "torus" in str(e.value)
    with pytest.raises(ValueError) as e:
        gol.Simulation(64, backend="cpu", boundary="dead", subtiles=2)
    assert "torus" in str(e.value)
    gol.Simulation(64, backend="cpu", boundary="torus", compat=True)  # the torus keeps compat mode
    # the torus-only HIP kernels (refused before any device is looked for)
    for kernel in ("temporal", "tile", "pipe", "resident", "lds"):
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="hip", boundary="dead", kernel=kernel)
        assert f"kernel {kernel!r} implements the torus only" in str(e.value)
    # the native engine refuses compat and sub-tiles on its own as well
    sim = gol.Simulation(64, backend="cpu")
    for field, value in [("compat", True), ("subtiles", 2)]:
        cfg = gol.native.EngineConfig()
        cfg.boundary = "dead"
        setattr(cfg, field, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(sim.geometry, cfg, sim.transport)
        assert "torus" in str(e.value)


# ----- views -----

def test_views_inside_and_across_the_edge(gol):
    N, W = 70, 130
    s = gol.Simulation(N, backend="cpu", boundary="dead", width=W, rule="B36/S23").init(5, seed=3)
    s.step(5)
    ref = oracle(random_board(N, W, 3), "B36/S23", 5)
    assert np.array_equal(s.window(0, 0, N, W), ref)
    assert np.array_equal(s.window(60, 100, 10, 30), ref[60:70, 100:130])
    dens = s.density(32, 64)
    assert dens.shape == (3, 3) and int(dens.sum()) == int(ref.sum()) and dens[2, 2] == ref[64:, 128:].sum()
    for rect in [(-1, 0, 5, 5), (0, -1, 5, 5), (66, 0, 5, 5), (0, 126, 5, 5)]:
        with pytest.raises(ValueError) as e:
            s.window(*rect)
        assert "bounded" in str(e.value) and f"({rect[0]}, {rect[1]})" in str(e.value)
        with pytest.raises(gol.native.GolError) as e:  # the engine on its own
            s.engine.window(*rect)
        assert "bounded" in str(e.value)
        with pytest.raises(ValueError):
            s.stamp(np.ones((5, 5), np.uint8), at=rect[:2])
        with pytest.raises(gol.native.GolError):
            s.engine.stamp(gol.ops.pattern_from_cells(np.ones((5, 5), np.uint8)), rect[0], rect[1], "or")
    # the torus wraps as before
    t = gol.Simulation(N, backend="cpu", width=W).init(5, seed=3)
    assert t.window(-1, -1, 5, 5).shape == (5, 5)
    # a stamp inside, and the centred one
    s.init(0).stamp(GLIDER, at=(67, 127))
    assert s.population() == 5 and s.window(67, 127, 3, 3).sum() == 5
    s.init(0).stamp(GLIDER)
    assert s.window((N - 3) // 2, (W - 3) // 2, 3, 3).sum() == 5


@pytest.mark.parametrize("H,W", [(64, 64), (100, 130)])
def test_gliders_leave(gol, H, W):
    """A glider 2 cells from each edge, heading out: it must not come back on the other side."""
    se = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8)  # moves down and right
    for name, pat, at in [("bottom-right", se, (H - 5, W - 5)), ("top-left", se[::-1, ::-1], (2, 2)),
                          ("top-right", se[::-1, :], (2, W - 5)), ("bottom-left", se[:, ::-1], (H - 5, 2))]:
        s = gol.Simulation(H, backend="cpu", boundary="dead", width=W, halo_depth=8).init(0)
        s.stamp(pat, at=at)
        start = s.board()
        far_r = slice(0, H // 3) if at[0] > H // 2 else slice(H - H // 3, H)
        far_c = slice(0, W // 3) if at[1] > W // 2 else slice(W - W // 3, W)
        for _ in range(8):
            s.step(8)
            b = s.board()
            assert b[far_r, :].sum() == 0 and b[:, far_c].sum() == 0, name
        assert np.array_equal(s.board(), oracle(start, "B3/S23", 64)), name


# ----- checkpoints -----

def test_checkpoint_keeps_the_boundary(gol, tmp_path):
    N, gens = 70, 9
    d = gol.Simulation(N, backend="cpu", boundary="dead").init(5, seed=4)
    d.step(gens)
    d.checkpoint(str(tmp_path / "d"))
    raw = (tmp_path / "d.gol").read_bytes()
    off = 8 + 7 * 8  # magic, then version, H, W, words_per_row, generation, seed, reserved[0]
    assert int.from_bytes(raw[off : off + 8], "little") == 1
    again = gol.Simulation(N, backend="cpu", boundary="dead").init(0)
    assert again.restore(str(tmp_path / "d")) == gens
    again.step(3)
    assert np.array_equal(again.board(), oracle(initial_board(5, N, 1, True, 4), "B3/S23", gens + 3))
    torus = gol.Simulation(N, backend="cpu").init(0)
    with pytest.raises(gol.native.GolError) as e:
        torus.restore(str(tmp_path / "d"))
    assert "boundary dead" in str(e.value) and "boundary torus" in str(e.value)


def test_torus_checkpoint_header_is_compatible(gol, tmp_path):
    """A torus run writes 0 where the boundary is kept, as every older file has: it loads in a torus run, and
    not on a bounded board."""
    N = 64
    t = gol.Simulation(N, backend="cpu").init(5, seed=4)
    t.checkpoint(str(tmp_path / "t"))
    raw = (tmp_path / "t.gol").read_bytes()
    off = 8 + 7 * 8
    assert int.from_bytes(raw[off : off + 8], "little") == 0
    fresh = gol.Simulation(N, backend="cpu").init(0)
    fresh.restore(str(tmp_path / "t"))
    assert np.array_equal(fresh.board(), initial_board(5, N, 1, True, 4))
    with pytest.raises(gol.native.GolError):
        gol.Simulation(N, backend="cpu", boundary="dead").init(0).restore(str(tmp_path / "t"))


# ----- RLE topology suffix -----

def py_suffix(field):
    """A small reader of the rule field's topology suffix, written here: (rule, topology, cols, rows) or None
    when the suffix must be refused."""
    if ":" not in field:
        return field, "", 0, 0
    rule, sfx = field.split(":", 1)
    if not sfx or sfx[0].upper() not in "TP":
        return None
    parts = sfx[1:].split(",")
    if len(parts) not in (1, 2) or not all(p.isdigit() and p.isascii() for p in parts):
        return None
    dims = [int(p) for p in parts]
    if 0 in dims:
        return None
    return rule, sfx[0].upper(), dims[0], dims[-1]


SUFFIXES = ["B3/S23", "B3/S23:P200,100", "B36/S23:T30,20", "B3/S23:P64", "B3/S23:t7", "B2/S:p5,9",
            "B3/S23:P0,100", "B3/S23:P100,0", "B3/S23:T0", "B3/S23:T30+5,20", "B3/S23:T30,20-2", "B3/S23:T30*,20",
            "B3/S23:K30,20", "B3/S23:C30,20", "B3/S23:S30", "B3/S23:X30", "B3/S23:", "B3/S23:P", "B3/S23:P,5",
            "B3/S23:P30,", "B3/S23:P30,20,10"]


@pytest.mark.parametrize("field", SUFFIXES)
def test_rle_suffix(gol, field):
    text = f"x = 3, y = 3, rule = {field}\nbob$2bo$3o!\n"
    want = py_suffix(field)
    if want is None:
        with pytest.raises(ValueError) as e:
            gol.native.parse_rle(text)
        assert "'" + field[field.index(":"):] + "'" in str(e.value)
        return
    p = gol.native.parse_rle(text)
    assert (p.rule, p.topology, p.bound_cols, p.bound_rows) == want
    assert ":" not in p.rule and p.rows == 3 and p.cols == 3
    out = gol.native.write_rle(p)
    header = out.splitlines()[0]
    if want[1]:
        assert header == f"x = 3, y = 3, rule = {want[0]}:{want[1]}{want[2]},{want[3]}"
    else:
        assert header == f"x = 3, y = 3, rule = {want[0]}"
    q = gol.native.parse_rle(out)
    assert (q.rule, q.topology, q.bound_cols, q.bound_rows) == want and np.array_equal(q.words, p.words)


def test_from_rle_adopts_the_topology(gol, tmp_path):
    path = tmp_path / "g.rle"
    path.write_text("x = 3, y = 3, rule = B3/S23:P40,30\nbob$2bo$3o!\n")
    s = gol.Simulation.from_rle(str(path), backend="cpu", at=(26, 36))  # no N: the file's 30 rows x 40 columns
    assert (s.decomposition.H, s.decomposition.W) == (30, 40) and s.stats()["boundary"] == "dead"
    start = s.board()
    s.step(40)
    assert np.array_equal(s.board(), oracle(start, "B3/S23", 40))
    s2 = gol.Simulation.from_rle(str(path), 64, backend="cpu")  # with N: a 64 x 64 board, still bounded
    assert (s2.decomposition.H, s2.decomposition.W) == (64, 64) and s2.stats()["boundary"] == "dead"
    assert gol.Simulation.from_rle(str(path), 64, backend="cpu", boundary="dead").stats()["boundary"] == "dead"
    with pytest.raises(ValueError) as e:
        gol.Simulation.from_rle(str(path), 64, backend="cpu", boundary="torus")
    assert "topology P" in str(e.value) and "torus" in str(e.value) and "dead" in str(e.value)
    with pytest.raises(ValueError) as e:
        gol.Simulation(64, backend="cpu").load_rle(str(path))
    assert "topology P" in str(e.value) and "torus" in str(e.value)
    # a torus suffix, and no suffix at all
    tpath = tmp_path / "t.rle"
    tpath.write_text("x = 3, y = 3, rule = B3/S23:T48\nbob$2bo$3o!\n")
    t = gol.Simulation.from_rle(str(tpath), backend="cpu")
    assert (t.decomposition.H, t.decomposition.W) == (48, 48) and t.stats()["boundary"] == "torus"
    with pytest.raises(ValueError):
        gol.Simulation.from_rle(str(tpath), 48, backend="cpu", boundary="dead")
    plain = tmp_path / "p.rle"
    plain.write_text(GLIDER)
    with pytest.raises(ValueError) as e:
        gol.Simulation.from_rle(str(plain), backend="cpu")
    assert "N" in str(e.value)
    assert gol.Simulation.from_rle(str(plain), 32, backend="cpu", boundary="dead").stats()["boundary"] == "dead"


def test_save_rle_names_the_plane(gol, tmp_path):
    s = gol.Simulation(30, backend="cpu", boundary="dead", width=40).init(0).stamp(GLIDER, at=(1, 1))
    s.save_rle(tmp_path / "whole.rle")
    assert (tmp_path / "whole.rle").read_text().splitlines()[0] == "x = 40, y = 30, rule = B3/S23:P40,30"
    s.save_rle(tmp_path / "part.rle", window=(0, 0, 5, 5))
    assert (tmp_path / "part.rle").read_text().splitlines()[0] == "x = 5, y = 5, rule = B3/S23"
    back = gol.Simulation.from_rle(str(tmp_path / "whole.rle"), backend="cpu", at=(0, 0))
    assert np.array_equal(back.board(), s.board()) and back.stats()["boundary"] == "dead"
    t = gol.Simulation(30, backend="cpu", width=40).init(0).stamp(GLIDER, at=(1, 1))
    t.save_rle(tmp_path / "torus.rle")
    assert (tmp_path / "torus.rle").read_text().splitlines()[0] == "x = 40, y = 30, rule = B3/S23"


# ----- CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_BOUNDARY",
              "GOL_PATTERN_FILE", "GOL_PATTERN_AT", "GOL_RLE_OUT"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


def test_cli_dead_dump(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path, GOL_BOUNDARY="dead", GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    _, _, cells = read_dump(os.path.join(tmp_path, "Rank_0_of_1.txt"))
    assert np.array_equal(cells, oracle(initial_board(5, 64), "B3/S23", 10))
    assert '"boundary": "dead"' in (tmp_path / "m.json").read_text()


def test_cli_dead_three_ranks(gol_bin, tmp_path):
    P, N, gens = 3, 48, 13
    r = _cli(gol_bin, [5, N, gens, 64, 1], tmp_path, GOL_BOUNDARY="dead", GOL_NRANKS=P, GOL_RULE="B36/S23")
    assert r.returncode == 0, r.stderr
    full = np.vstack([read_dump(os.path.join(tmp_path, f"Rank_{q}_of_{P}.txt"))[2] for q in range(P)])
    assert np.array_equal(full, oracle(initial_board(5, N, P, True), "B36/S23", gens))


def test_cli_torus_is_the_default(gol_bin, tmp_path):
    outs = []
    for i, env in enumerate([{}, {"GOL_BOUNDARY": "torus"}]):
        r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path / str(i), **env)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        outs.append((tmp_path / str(i) / "Rank_0_of_1.txt").read_bytes())
    assert outs[0] == outs[1]


def test_cli_banana_rejected(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path, GOL_BOUNDARY="banana")
    assert r.returncode != 0 and "'banana'" in r.stderr and "torus or dead" in r.stderr
    assert not list(tmp_path.glob("Rank_*"))  # before any rank started


def test_cli_pattern_file_topology(gol_bin, tmp_path):
    pat = tmp_path / "g.rle"
    pat.write_text("x = 3, y = 3, rule = B3/S23:P999,999\nbob$2bo$3o!\n")  # (the suffix's size is ignored: worldSize governs)
    N, gens = 32, 60
    r = _cli(gol_bin, [0, N, gens, 64, 1], tmp_path / "a", GOL_PATTERN_FILE=pat, GOL_PATTERN_AT="27,27",
             GOL_RLE_OUT=tmp_path / "a" / "out.rle", GOL_METRICS_JSON=tmp_path / "a" / "m.json")
    assert r.returncode == 0, r.stderr
    assert '"boundary": "dead"' in (tmp_path / "a" / "m.json").read_text()
    start = np.zeros((N, N), np.uint8)
    start[27:30, 27:30] = [[0, 1, 0], [0, 0, 1], [1, 1, 1]]
    _, _, cells = read_dump(os.path.join(tmp_path, "a", "Rank_0_of_1.txt"))
    assert np.array_equal(cells, oracle(start, "B3/S23", gens))
    assert (tmp_path / "a" / "out.rle").read_text().splitlines()[0] == f"x = {N}, y = {N}, rule = B3/S23:P{N},{N}"
    # GOL_BOUNDARY that agrees, and one that does not
    assert _cli(gol_bin, [0, N, 4, 64, 0], tmp_path / "b", GOL_PATTERN_FILE=pat, GOL_BOUNDARY="dead").returncode == 0
    r = _cli(gol_bin, [0, N, 4, 64, 1], tmp_path / "c", GOL_PATTERN_FILE=pat, GOL_BOUNDARY="torus")
    assert r.returncode != 0 and "topology P" in r.stderr and "torus" in r.stderr
    assert not list((tmp_path / "c").glob("Rank_*"))
    # a rectangle across the edge ends the run, naming the rectangle and the board
    r = _cli(gol_bin, [0, N, 4, 64, 0], tmp_path / "d", GOL_PATTERN_FILE=pat, GOL_PATTERN_AT="30,30")
    assert r.returncode != 0 and "(30, 30)" in r.stderr and "bounded 32 x 32" in r.stderr
