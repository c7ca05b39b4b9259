"""Pattern files, stamping, windows and density maps on the CPU backend, the Python API and the CLI, against
numpy on ``board()`` / ``initial_board`` and an independent RLE reader and writer written here."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_step, numpy_step_rule, parse_rle, write_rle
from gol_amd.utils import read_dump

GLIDER_BODY = "bob$2bo$3o!"
GLIDER = "x = 3, y = 3\n" + GLIDER_BODY + "\n"
GLIDER_CELLS = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8)
MODES = ["or", "replace", "xor", "clear"]


# ----- an independent RLE reader and writer (pure Python) -----

def py_parse_rle(text):
    lines = [ln for ln in text.splitlines() if ln.strip() and not ln.lstrip().startswith("#")]
    m = re.match(r"\s*x\s*=\s*(\d+)\s*,\s*y\s*=\s*(\d+)\s*(?:,\s*rule\s*=\s*(\S+))?\s*$", lines[0], re.I)
    x, y, rule = int(m.group(1)), int(m.group(2)), m.group(3) or ""
    cells = np.zeros((y, x), np.uint8)
    r = c = 0
    for count, tag in re.findall(r"(\d*)([bo$!])", "".join(lines[1:]).split("!")[0] + "!"):
        n = int(count or 1)
        if tag == "o":
            cells[r, c : c + n] = 1
        if tag in "bo":
            c += n
        elif tag == "$":
            r, c = r + n, 0
    return cells, rule


def py_write_rle(cells, rule=""):
    y, x = cells.shape
    toks, gap = [], 0
    for row in cells:
        live = np.flatnonzero(row)
        if len(live) == 0:
            gap += 1
            continue
        if gap:
            toks.append((gap, "$"))
        gap = 1
        c = 0
        while c <= live[-1]:
            e = c
            while e <= live[-1] and row[e] == row[c]:
                e += 1
            toks.append((e - c, "o" if row[c] else "b"))
            c = e
    toks.append((1, "!"))
    out, line = [f"x = {x}, y = {y}" + (f", rule = {rule}" if rule else "")], ""
    for n, tag in toks:
        t = (str(n) if n > 1 else "") + tag
        if len(line) + len(t) > 70:
            out.append(line)
            line = ""
        line += t
    return "\n".join(out + [line]) + "\n"


def rand_cells(rows, cols, seed, density=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < density).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (64, 64), (65, 3), (70, 200), (37, 70)])
@pytest.mark.parametrize("density", [0.03, 0.5, 0.97])
def test_native_and_python_rle_agree(shape, density):
    cells = rand_cells(*shape, seed=shape[0] * 1000 + shape[1], density=density)
    cells[0, 0] = cells[-1, -1] = 1  # (keeps the bounding box; both writers drop trailing dead rows)
    for rule in ("", "B36/S23"):
        text = write_rle(cells, rule)
        assert text == py_write_rle(cells, rule)  # native writer == Python writer, byte for byte
        got, got_rule = py_parse_rle(text)  # native writer -> Python reader
        assert np.array_equal(got, cells) and got_rule == rule
        got, got_rule = parse_rle(py_write_rle(cells, rule))  # Python writer -> native reader
        assert np.array_equal(got, cells) and got_rule == rule
        assert all(len(ln) <= 70 for ln in text.splitlines()[1:]) and text.rstrip().endswith("!")


def test_parse_rle_forms_and_errors():
    cells, rule = parse_rle("#C glider\nx = 3, y = 3, rule = 23/3\nbo$2bo$\n3o! ignored")
    assert np.array_equal(cells, GLIDER_CELLS) and rule == "B3/S23"
    assert np.array_equal(parse_rle("x = 3, y = 6\n3o3$obo!")[0], np.array(
        [[1, 1, 1], [0, 0, 0], [0, 0, 0], [1, 0, 1], [0, 0, 0], [0, 0, 0]], np.uint8))
    for bad, needle in [("bob$2bo$3o!", "header"), ("x = 3, y = 3\n4o!", "passes x"), ("x = 3, y = 3\no4$!", "passes y"),
                        ("x = 3, y = 3\nbxb!", "'x'"), ("x = 3, y = 3\n99999999999999999999o!", "overflow"),
                        ("x = 3, y = 3\n3o", "missing '!'"), ("x = 3, y = 3, rule = B0/S\no!", "B0")]:
        with pytest.raises(ValueError) as e:
            parse_rle(bad)
        assert needle in str(e.value), (bad, str(e.value))


# ----- numpy oracles -----

def np_window(board, r0, c0, rows, cols):
    return np.take(np.take(board, np.arange(r0, r0 + rows), axis=0, mode="wrap"), np.arange(c0, c0 + cols), axis=1,
                   mode="wrap")


def np_density(board, br, bc):
    H, W = board.shape
    gh, gw = -(-H // br), -(-W // bc)
    pad = np.zeros((gh * br, gw * bc), np.uint32)
    pad[:H, :W] = board
    return pad.reshape(gh, br, gw, bc).sum(axis=(1, 3)).astype(np.uint32)


def np_stamp(board, pat, r0, c0, mode):
    out = board.copy()
    idx = np.ix_((r0 + np.arange(pat.shape[0])) % board.shape[0], (c0 + np.arange(pat.shape[1])) % board.shape[1])
    cur = out[idx]
    out[idx] = {"or": cur | pat, "replace": pat, "xor": cur ^ pat, "clear": cur & (1 - pat)}[mode]
    return out


def _sim(gol, N, **kw):
    kw.setdefault("backend", "cpu")
    return gol.Simulation(N, **kw)


# ----- one rank -----

@pytest.mark.parametrize("k", [1, 5, 16])
def test_glider_crosses_the_corner(gol, k):
    """A glider stamped across the corner of a 64^2 torus moves one cell down and right every 4 generations."""
    N = 64
    s = _sim(gol, N).init(0)
    s.stamp(GLIDER, at=(62, 62))
    assert s.population() == 5
    assert np.array_equal(s.window(62, 62, 3, 3), GLIDER_CELLS)
    assert np.array_equal(s.board(), np_stamp(np.zeros((N, N), np.uint8), GLIDER_CELLS, 62, 62, "or"))
    s.step(4 * k)
    assert s.population() == 5
    assert np.array_equal(s.window(62 + k, 62 + k, 3, 3), GLIDER_CELLS)
    assert np.array_equal(s.board(), np_stamp(np.zeros((N, N), np.uint8), GLIDER_CELLS, 62 + k, 62 + k, "or"))


@pytest.mark.parametrize("N,W", [(1, 0), (3, 0), (63, 0), (64, 0), (65, 0), (137, 0), (100, 200)])
def test_window_and_density_vs_numpy(gol, N, W):
    s = _sim(gol, N, width=W).init(5, seed=N)
    s.step(3)
    board = s.board()
    H, Wd = board.shape
    wins = [(0, 0, 1, 1), (0, 0, H, Wd), (H // 2, Wd // 2, H, Wd), (-1, -1, min(H, 3), min(Wd, 3)),
            (H - 1, 5, min(H, 2), 1), (7, Wd - 1, 1, min(Wd, 2)), (5 * H + 2, -3 * Wd + 1, max(1, H - 1), max(1, Wd - 1))]
    if Wd >= 71:
        wins += [(3, 63, 5, 2), (0, 60, H, 11)]
    for r0, c0, rows, cols in wins:
        got = s.window(r0, c0, rows, cols)
        assert got.dtype == np.uint8 and got.shape == (rows, cols)
        assert np.array_equal(got, np_window(board, r0, c0, rows, cols)), (r0, c0, rows, cols)
    for br, bc in [(1, 64), (7, 64), (64, 128), (H, 64 * -(-Wd // 64)), (H + 5, 192)]:
        got = s.density(br, bc)
        assert got.dtype == np.uint32 and np.array_equal(got, np_density(board, br, bc)), (br, bc)
    assert int(s.density(64).sum()) == s.population() == int(board.sum())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,at", [(137, (0, 0)), (137, (1, 63)), (137, (64, 1)), (137, (120, 100)), (200, (190, 150)),
                                   (70, (69, 69)), (37, (5, 0))])
def test_stamp_modes_vs_numpy(gol, mode, N, at):
    """A 37 x 70 random pattern at word-aligned and unaligned offsets, across both seams, on boards as large as
    the pattern in one or both directions; then 9 generations (stale ghost cells would show)."""
    pat = rand_cells(37, 70, seed=3)
    W = max(N, 70)
    s = _sim(gol, N, width=W).init(5, seed=N)
    s.step(2)
    before = s.board()
    s.stamp(pat, at=at, mode=mode)
    want = np_stamp(before, pat, at[0], at[1], mode)
    assert np.array_equal(s.board(), want)
    s.step(9)
    assert np.array_equal(s.board(), numpy_step(want, 9))


def test_stamp_inputs_and_center(gol, tmp_path):
    N = 64
    path = tmp_path / "glider.rle"
    path.write_text("x = 3, y = 3, rule = B3/S23\n" + GLIDER_BODY + "\n")
    want = np_stamp(np.zeros((N, N), np.uint8), GLIDER_CELLS, 30, 30, "or")
    for pattern in (str(path), path, GLIDER, GLIDER_CELLS, GLIDER_CELLS.tolist()):
        s = _sim(gol, N).init(0)
        assert s.stamp(pattern) is s  # centred: ((64 - 3) // 2, (64 - 3) // 2) = (30, 30)
        assert np.array_equal(s.board(), want)
    s = _sim(gol, N).init(5, seed=1).load_rle(path, at=(1, 2))  # an empty board, then the pattern
    assert s.generation == 0 and np.array_equal(s.board(), np_stamp(np.zeros((N, N), np.uint8), GLIDER_CELLS, 1, 2, "or"))
    with pytest.raises(FileNotFoundError):
        s.stamp(str(tmp_path / "missing.rle"))


def test_save_rle_and_from_rle(gol, tmp_path):
    N = 70
    s = _sim(gol, N, rule="B36/S23").init(5, seed=2)
    s.step(4)
    s.save_rle(tmp_path / "all.rle")
    s.save_rle(tmp_path / "win.rle", window=(60, 65, 20, 10))
    cells, rule = parse_rle((tmp_path / "all.rle").read_text())
    assert rule == "B36/S23" and np.array_equal(cells, s.board())
    cells, rule = py_parse_rle((tmp_path / "win.rle").read_text())
    assert rule == "B36/S23" and np.array_equal(cells, np_window(s.board(), 60, 65, 20, 10))
    # from_rle takes the rule from the file
    t = gol.Simulation.from_rle(tmp_path / "all.rle", N, backend="cpu", at=(0, 0))
    assert t.stats()["rule"] == "B36/S23" and np.array_equal(t.board(), s.board())
    t.step(5)
    s.step(5)
    assert np.array_equal(t.board(), s.board())
    assert np.array_equal(t.board(), numpy_step_rule(initial_board(5, N, 1, True, 2), "B36/S23", 9))
    with pytest.raises(ValueError) as e:
        gol.Simulation.from_rle(tmp_path / "all.rle", N, backend="cpu", rule="B3/S23")
    assert "B36/S23" in str(e.value) and "B3/S23" in str(e.value)


def test_error_cases(gol, tmp_path):
    s = _sim(gol, 64).init(5, seed=1)
    board = s.board()
    errors = (ValueError, gol.native.GolError)
    for pat in (np.ones((65, 3), np.uint8), np.ones((3, 65), np.uint8)):  # larger than the board
        with pytest.raises(errors) as e:
            s.stamp(pat, at=(0, 0))
        assert "larger than the board" in str(e.value)
        with pytest.raises(gol.native.GolError) as e:  # the native engine refuses it on its own too
            s.engine.stamp(gol.ops.pattern_from_cells(pat), 0, 0, "or")
        assert "larger than the board" in str(e.value)
    for bc in (0, 1, 63, 65, 100):
        with pytest.raises(errors) as e:
            s.density(8, bc)
        assert "64" in str(e.value)
        with pytest.raises(gol.native.GolError):
            s.engine.density(8, bc)
    with pytest.raises(errors):
        s.density(0, 64)
    with pytest.raises(errors):
        s.density(100)  # block_cols defaults to block_rows
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 65, 1), (0, 0, 1, 65)):
        with pytest.raises(errors):
            s.window(*win)
    with pytest.raises(errors):
        s.stamp(GLIDER, mode="and")
    with pytest.raises(errors):
        s.stamp(GLIDER, at="corner")
    c = _sim(gol, 64, compat=True).init(5, seed=1)
    with pytest.raises(errors) as e:
        c.stamp(GLIDER)
    assert "compat" in str(e.value)
    with pytest.raises(gol.native.GolError) as e:
        c.engine.stamp(gol.native.parse_rle(GLIDER), 0, 0, "or")
    assert "compat" in str(e.value)
    assert np.array_equal(c.window(0, 0, 64, 64), c.board())  # (reading stays allowed)
    # a file under another rule
    path = tmp_path / "hl.rle"
    path.write_text("x = 3, y = 3, rule = B36/S23\n" + GLIDER_BODY + "\n")
    with pytest.raises(ValueError) as e:
        s.load_rle(path)
    assert "B36/S23" in str(e.value) and "B3/S23" in str(e.value)
    assert np.array_equal(s.board(), board)  # nothing above changed the board


# ----- thread ranks -----

def _thread_views(gol, P, N, **kw):
    per_rank = not kw.get("global_mode", False)
    H, W = (N * P if per_rank else N), N
    pat = rand_cells(37, 45, seed=5)
    at = (H - 10, W - 20)               # crosses both seams, and the boundary between the last and the first rank
    win = (H - 30, W - 25, 70, 50)      # likewise (70 rows: three ranks' rows in 1-D with N = 50)
    mid = (H // 2 - 30, W // 2 - 20)    # crosses the inner rank boundaries
    ts = gol.parallel.thread_transports(P)
    out, errs = [None] * P, []

    def worker(r):
        try:
            s = gol.Simulation(N, ts[r], backend="cpu", **kw).init(5, seed=11)
            s.step(3)
            res = {"w0": s.window(*win), "d0": s.density(7, 64), "full0": s.window(0, 0, H, W)}
            s.stamp(pat, at=at, mode="xor")
            s.stamp(pat, at=mid, mode="replace")
            res["full1"] = s.window(0, 0, H, W)
            s.step(9)
            res["full2"] = s.window(H // 2, W // 2, H, W)
            res["d2"] = s.density(64, 64)
            res["pop"] = s.population()
            out[r] = res
        except Exception as e:  # reported below
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not errs, errs
    for r in range(1, P):  # every rank gets the identical full result
        for key in out[0]:
            assert np.array_equal(out[r][key], out[0][key]), (r, key)
    b0 = numpy_step(initial_board(5, N, P, per_rank, 11), 3)
    assert np.array_equal(out[0]["full0"], b0)
    assert np.array_equal(out[0]["w0"], np_window(b0, *win))
    assert np.array_equal(out[0]["d0"], np_density(b0, 7, 64))
    b1 = np_stamp(np_stamp(b0, pat, at[0], at[1], "xor"), pat, mid[0], mid[1], "replace")
    assert np.array_equal(out[0]["full1"], b1)
    b2 = numpy_step(b1, 9)
    assert np.array_equal(out[0]["full2"], np_window(b2, H // 2, W // 2, H, W))
    assert np.array_equal(out[0]["d2"], np_density(b2, 64, 64)) and out[0]["pop"] == int(b2.sum())


def test_thread_ranks_1d(gol):
    _thread_views(gol, 3, 50, halo_depth=4)


def test_thread_ranks_2x2(gol):
    _thread_views(gol, 4, 128, halo_depth=4, decomp="2d", grid="2x2", global_mode=True)


def test_bad_call_raises_on_every_rank(gol):
    """Arguments are validated before any communication: every rank raises, none hangs."""
    P = 2
    ts = gol.parallel.thread_transports(P)
    errs = [[] for _ in range(P)]

    def worker(r):
        s = gol.Simulation(32, ts[r], backend="cpu").init(5, seed=1)
        for call in (lambda: s.engine.window(0, 0, 65, 1), lambda: s.engine.density(8, 100),
                     lambda: s.engine.stamp(gol.ops.pattern_from_cells(np.ones((3, 33), np.uint8)), 0, 0, "or")):
            try:
                call()
            except Exception as e:
                errs[r].append(e)

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(len(e) == 3 for e in errs), errs


# ----- CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_PATTERN_FILE",
              "GOL_PATTERN_AT", "GOL_RLE_OUT"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


def test_cli_pattern_file(gol_bin, tmp_path):
    rle = tmp_path / "glider.rle"
    rle.write_text("#C a glider\n" + GLIDER)
    # at a position, across the corner of the torus
    r = _cli(gol_bin, [0, 64, 8, 64, 1], tmp_path / "a", GOL_PATTERN_FILE=rle, GOL_PATTERN_AT="62,63")
    assert r.returncode == 0, r.stderr
    _, _, cells = read_dump(os.path.join(tmp_path, "a", "Rank_0_of_1.txt"))
    assert np.array_equal(cells, np_stamp(np.zeros((64, 64), np.uint8), GLIDER_CELLS, 64, 65, "or"))
    # centred, on top of the positional pattern, over two thread ranks (the board is 128 x 64)
    r = _cli(gol_bin, [5, 64, 6, 64, 1], tmp_path / "b", GOL_PATTERN_FILE=rle, GOL_NRANKS=2)
    assert r.returncode == 0, r.stderr
    want = numpy_step(np_stamp(initial_board(5, 64, 2), GLIDER_CELLS, (128 - 3) // 2, (64 - 3) // 2, "or"), 6)
    got = np.vstack([read_dump(os.path.join(tmp_path, "b", f"Rank_{q}_of_2.txt"))[2] for q in range(2)])
    assert np.array_equal(got, want)
    # unset: nothing changes
    r = _cli(gol_bin, [5, 64, 6, 64, 1], tmp_path / "c")
    assert np.array_equal(read_dump(os.path.join(tmp_path, "c", "Rank_0_of_1.txt"))[2], numpy_step(initial_board(5, 64), 6))
    # errors end the run non-zero, with the reason
    r = _cli(gol_bin, [0, 64, 1, 64, 0], tmp_path / "d", GOL_PATTERN_FILE=tmp_path / "none.rle")
    assert r.returncode != 0 and "none.rle" in r.stderr
    r = _cli(gol_bin, [0, 64, 1, 64, 0], tmp_path / "d", GOL_PATTERN_FILE=rle, GOL_PATTERN_AT="7")
    assert r.returncode != 0 and "GOL_PATTERN_AT" in r.stderr
    (tmp_path / "bad.rle").write_text("x = 3, y = 3\nbob$2bq$3o!\n")
    r = _cli(gol_bin, [0, 64, 1, 64, 0], tmp_path / "d", GOL_PATTERN_FILE=tmp_path / "bad.rle")
    assert r.returncode != 0 and "'q'" in r.stderr and "bad.rle" in r.stderr
    r = _cli(gol_bin, [0, 2, 1, 64, 0], tmp_path / "d", GOL_PATTERN_FILE=rle)
    assert r.returncode != 0 and "larger than the board" in r.stderr


def test_cli_rule_from_file(gol_bin, tmp_path):
    pat = rand_cells(20, 30, seed=8)
    rle = tmp_path / "hl.rle"
    rle.write_text(py_write_rle(pat, "23/36"))  # HighLife in the S/B form
    start = np_stamp(initial_board(5, 64), pat, 3, 4, "or")
    # GOL_RULE unset: the file's rule is the run's
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path / "a", GOL_PATTERN_FILE=rle, GOL_PATTERN_AT="3,4", GOL_VERBOSE=1)
    assert r.returncode == 0 and "rule B36/S23" in r.stderr, r.stderr
    _, _, cells = read_dump(os.path.join(tmp_path, "a", "Rank_0_of_1.txt"))
    assert np.array_equal(cells, numpy_step_rule(start, "B36/S23", 10))
    assert not np.array_equal(cells, numpy_step(start, 10))  # (the rule does matter on this board)
    # the same rule asked for, in another spelling: fine
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path / "b", GOL_PATTERN_FILE=rle, GOL_PATTERN_AT="3,4", GOL_RULE="highlife")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_dump(os.path.join(tmp_path, "b", "Rank_0_of_1.txt"))[2], cells)
    # a different one: the run ends non-zero and names both
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path / "c", GOL_PATTERN_FILE=rle, GOL_RULE="B3/S23")
    assert r.returncode != 0 and "B36/S23" in r.stderr and "B3/S23" in r.stderr, r.stderr
    assert not list((tmp_path / "c").glob("Rank_*"))  # before any rank started


def test_cli_rle_out(gol_bin, tmp_path):
    for i, (env, P) in enumerate([({}, 1), ({"GOL_NRANKS": 3, "GOL_RULE": "B36/S23"}, 3),
                                  ({"GOL_NRANKS": 4, "GOL_GLOBAL": 1, "GOL_DECOMP": "2d", "GOL_GRID": "2x2"}, 4)]):
        cwd = tmp_path / str(i)
        N = 128 if P == 4 else 40
        r = _cli(gol_bin, [5, N, 7, 64, 1], cwd, GOL_RLE_OUT="final.rle", **env)
        assert r.returncode == 0, r.stderr
        dump = np.vstack([read_dump(os.path.join(cwd, f"Rank_{q}_of_{P}.txt"))[2] for q in range(P)])
        cells, rule = parse_rle((cwd / "final.rle").read_text())
        assert rule == env.get("GOL_RULE", "B3/S23") and np.array_equal(cells, dump)
        assert np.array_equal(py_parse_rle((cwd / "final.rle").read_text())[0], dump)
    # refused above 2^26 cells, before anything runs
    r = _cli(gol_bin, [0, 8200, 0, 64, 0], tmp_path / "big", GOL_RLE_OUT="final.rle")
    assert r.returncode != 0 and "2^26" in r.stderr and "GOL_RLE_OUT" in r.stderr
    assert not (tmp_path / "big" / "final.rle").exists()
