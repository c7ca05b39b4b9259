"""Von Neumann (``V``) and hexagonal (``H``) rules without a GPU: rule strings, the CPU backend against the numpy oracles
(which count neighbours by shifted adds over the literal 3 x 3 masks), thread ranks, RLE, the CLI and checkpoints."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from gol_amd.ops import (
    initial_board,
    numpy_census,
    numpy_signatures,
    numpy_step_rule,
    numpy_step_rule_bounded,
    parse_rle,
    parse_rule,
    parse_rule_nbhd,
    random_board,
    rule_string,
    torch_step_rule,
    write_rle,
)
from gol_amd.utils import read_dump

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEX, VON = "B2/S34H", "B13/S13V"
BOUNDARIES = ["torus", "dead"]
# the neighbourhoods as literals (rows downward, columns rightward)
MASKS = {"V": [[0, 1, 0], [1, 0, 1], [0, 1, 0]], "H": [[1, 1, 0], [1, 0, 1], [0, 1, 1]]}


def _random_rules():
    rng = np.random.default_rng(3)
    out = []
    for sfx, top in (("V", 4), ("H", 6)):
        birth, survive = (int(v) for v in rng.integers(0, 2 << top, size=2))
        out.append(rule_string((birth & ~1 | 2, survive, sfx)))
    return out


RULES = [HEX, VON, "B1/SH", "B1/SV"] + _random_rules()


def _step(boundary):
    return numpy_step_rule_bounded if boundary == "dead" else numpy_step_rule


# ----- rule strings -----

@pytest.mark.parametrize("text,canon", [("B2/S34H", "B2/S34H"), ("s43/b2h", "B2/S34H"), ("S31/B31v", "B13/S13V"),
                                        ("b1/sV", "B1/SV"), ("B/S0h", "B/S0H"), ("B654321/S6543210H", "B123456/S0123456H")])
def test_round_trips(gol, text, canon):
    assert gol.Simulation(16, backend="cpu", rule=text).stats()["rule"] == canon
    assert rule_string(text) == canon and rule_string(canon) == canon
    b, s, n = gol.native.parse_rule_nbhd(text)
    assert (b, s, n) == parse_rule_nbhd(text) and n == canon[-1]
    assert tuple(gol.native.parse_rule(text)) == parse_rule(text) == (b, s)
    assert rule_string((b, s, n)) == canon


def test_moore_strings_mean_what_they_meant(gol):
    assert parse_rule_nbhd("B36/S23") == (0x48, 0xC, "") and parse_rule("highlife") == (0x48, 0xC)
    assert tuple(gol.native.parse_rule_nbhd("B3/S23")) == (8, 12, "")
    assert rule_string("B3/S23") == "B3/S23" and rule_string((8, 12)) == "B3/S23"


@pytest.mark.parametrize("bad", ["B5/S2V", "B2/S5V", "B7/S2H", "B2/S7H", "B0/SV", "B3/S23VH", "B3/S23 V", "B3V/S23"])
def test_rejections(gol, bad):
    with pytest.raises(ValueError) as e:
        gol.native.parse_rule(bad)
    assert f"'{bad}'" in str(e.value)
    with pytest.raises(ValueError):
        gol.Simulation(16, backend="cpu", rule=bad)
    with pytest.raises(ValueError):
        parse_rule_nbhd(bad)


def test_rejection_names_the_range(gol):
    with pytest.raises(ValueError) as e:
        gol.native.parse_rule("B5/S2V")
    assert "von Neumann" in str(e.value) and "0 to 4" in str(e.value)
    with pytest.raises(ValueError) as e:
        gol.native.parse_rule("B7/S2H")
    assert "hexagonal" in str(e.value) and "0 to 6" in str(e.value)


# ----- the masks, as literals -----

@pytest.mark.parametrize("sfx", ["V", "H"])
def test_literal_masks(gol, sfx):
    """One live cell at the centre of a 5 x 5 torus under B1/S: after one generation, the mask itself."""
    start = np.zeros((5, 5), np.uint8)
    start[2, 2] = 1
    want = np.zeros((5, 5), np.uint8)
    want[1:4, 1:4] = np.array(MASKS[sfx], np.uint8)
    rule = f"B1/S{sfx}"
    assert np.array_equal(numpy_step_rule(start, rule, 1), want)
    assert np.array_equal(numpy_step_rule_bounded(start, rule, 1), want)
    assert np.array_equal(torch_step_rule(start, rule, 1).numpy(), want)
    for boundary in BOUNDARIES:
        s = gol.Simulation(5, backend="cpu", rule=rule, boundary=boundary).init(0)
        s.set_board(start)
        s.step(1)
        assert np.array_equal(s.board(), want)


# ----- the CPU backend against numpy -----

@functools.lru_cache(maxsize=None)
def reference(N, rule, boundary, gens):
    b = random_board(N, N, 7)
    if N > 3:
        assert not np.array_equal(_step(boundary)(b, rule, 1), _step(boundary)(b, rule_string(rule)[:-1], 1))
    counts, board = numpy_census(b, rule, gens, bounded=boundary == "dead", return_board=True)
    sigs = numpy_signatures(b, rule, gens, bounded=boundary == "dead")
    board.setflags(write=False)
    return board, counts, sigs


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200])
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("rule", RULES)
def test_cpu_vs_numpy(gol, rule, boundary, N):
    gens = 11
    board, counts, sigs = reference(N, rule, boundary, gens)
    s = gol.Simulation(N, backend="cpu", rule=rule, boundary=boundary, halo_depth=4).init(5, seed=7)
    s.step(gens)
    assert s.stats()["rule"] == rule
    assert np.array_equal(s.board(), board)
    c = gol.Simulation(N, backend="cpu", rule=rule, boundary=boundary, halo_depth=4, census=True).init(5, seed=7)
    c.step(gens)
    assert np.array_equal(c.census()[1], counts) and int(counts[-1]) == c.population()
    g = gol.Simulation(N, backend="cpu", rule=rule, boundary=boundary, halo_depth=4, signature=True).init(5, seed=7)
    g.step(gens)
    start, got, pops = g.signatures()
    assert start == 0 and np.array_equal(got, sigs) and np.array_equal(pops, counts) and int(got[-1]) == g.signature()


def test_torch_oracle_agrees():
    b = random_board(65, 70, 3)
    for rule in (HEX, VON):
        assert np.array_equal(torch_step_rule(b, rule, 5).numpy(), numpy_step_rule(b, rule, 5))


def test_find_cycle_cpu(gol):
    rule, N = HEX, 64
    board = np.zeros((N, N), np.uint8)
    board[30:34, 30:34] = np.array([[1, 1, 0, 0], [1, 1, 1, 1], [0, 1, 1, 0], [1, 0, 0, 0]], np.uint8)
    seen, b, want = {board.tobytes(): 0}, board, None
    for g in range(1, 2001):
        b = numpy_step_rule(b, rule, 1)
        if b.tobytes() in seen:
            want = (seen[b.tobytes()], g - seen[b.tobytes()])
            break
        seen[b.tobytes()] = g
    assert want is not None
    s = gol.Simulation(N, backend="cpu", rule=rule, halo_depth=8, signature=True).init(0)
    s.set_board(board)
    got = s.find_cycle(2000, chunk=50)
    assert got is not None and (got.transient, got.period) == want


# ----- thread ranks -----

def _run_threads(gol, N, P, gens, rules, **kw):
    ts = gol.parallel.thread_transports(P)
    boards, errs = [None] * P, [None] * P

    def worker(r):
        try:
            s = gol.Simulation(N, ts[r], backend="cpu", global_mode=True, rule=rules[r], **kw).init(5, seed=99)
            s.step(gens)
            boards[r] = (s.geometry.row0, s.geometry.col0, s.board())
        except Exception as e:  # looked at by the caller
            errs[r] = e

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th)
    return boards, errs


@pytest.mark.parametrize("P,kw", [(3, {}), (4, {"decomp": "2d", "grid": "2x2"})], ids=["P3", "2x2"])
@pytest.mark.parametrize("rule,boundary", [(HEX, "torus"), (VON, "torus"), (HEX, "dead"), (VON, "dead")])
def test_thread_ranks_equal_one_rank(gol, rule, boundary, P, kw):
    N, gens = 128, 19
    one = gol.Simulation(N, backend="cpu", rule=rule, boundary=boundary, halo_depth=4).init(5, seed=99)
    one.step(gens)
    boards, errs = _run_threads(gol, N, P, gens, [rule] * P, boundary=boundary, halo_depth=4, **kw)
    assert not any(errs), errs
    full = np.full((N, N), 255, np.uint8)
    for r0, c0, b in boards:
        full[r0 : r0 + b.shape[0], c0 : c0 + b.shape[1]] = b
    assert np.array_equal(full, one.board())
    assert np.array_equal(full, _step(boundary)(initial_board(5, N, 1, True, 99), rule, gens))


def test_rank_neighbourhood_mismatch_raises_everywhere(gol):
    _, errs = _run_threads(gol, 64, 2, 1, ["B2/S34H", "B2/S34"])
    assert all(e is not None and "rule" in str(e) for e in errs), errs


# ----- RLE -----

def test_rle(gol, tmp_path):
    cells, rule = parse_rle("x = 3, y = 2, rule = B2/S34H\nobo$3o!\n")
    assert rule == HEX and cells.tolist() == [[1, 0, 1], [1, 1, 1]]
    assert parse_rle("x = 1, y = 1, rule = 34/2H\no!")[1] == HEX
    assert parse_rle("x = 1, y = 1, rule = 13/13v\no!")[1] == VON
    assert "rule = B2/S34H\n" in write_rle(cells, "s34/b2h")
    assert parse_rle(write_rle(cells, HEX))[1] == HEX
    for topo, boundary in (("T", "torus"), ("P", "dead")):
        path = tmp_path / f"{topo}.rle"
        path.write_text(f"x = 3, y = 2, rule = B2/S34H:{topo}64,64\nobo$3o!\n")
        s = gol.Simulation.from_rle(str(path), backend="cpu")
        st = s.stats()
        assert st["rule"] == HEX and st["boundary"] == boundary and s.board().shape == (64, 64), st
        start = s.board()
        s.step(5)
        assert np.array_equal(s.board(), _step(boundary)(start, HEX, 5))
        out = tmp_path / f"{topo}_out.rle"
        s.save_rle(str(out))
        header = out.read_text().splitlines()[0]
        assert "rule = B2/S34H" in header and (boundary == "torus" or header.endswith(":P64,64")), header
        again = gol.Simulation.from_rle(str(out), backend="cpu", **({} if boundary == "dead" else {"N": 64}))
        assert again.stats()["rule"] == HEX
    with pytest.raises(ValueError):
        gol.Simulation(64, backend="cpu", rule="B2/S34").load_rle(str(tmp_path / "T.rle"))


# ----- CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_PATTERN_FILE",
              "GOL_PATTERN_AT", "GOL_RLE_OUT", "GOL_COMPAT"):
        e.pop(k, None)
    e["GOL_BACKEND"] = "cpu"
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


def _load(cwd, P):
    parts = sorted((read_dump(os.path.join(cwd, f"Rank_{r}_of_{P}.txt"))[1:] for r in range(P)), key=lambda t: t[0])
    return np.vstack([c for _, c in parts])


def test_cli_ranks_identical(gol_bin, tmp_path):
    N, gens = 96, 10
    r = _cli(gol_bin, [5, N, gens, 64, 1], tmp_path / "p1", GOL_RULE=HEX, GOL_GLOBAL=1)
    assert r.returncode == 0, r.stderr
    r = _cli(gol_bin, [5, N, gens, 64, 1], tmp_path / "p3", GOL_RULE=HEX, GOL_GLOBAL=1, GOL_NRANKS=3)
    assert r.returncode == 0, r.stderr
    one, three = _load(tmp_path / "p1", 1), _load(tmp_path / "p3", 3)
    assert np.array_equal(one, three)
    assert np.array_equal(one, numpy_step_rule(initial_board(5, N), HEX, gens))
    assert not np.array_equal(one, numpy_step_rule(initial_board(5, N), "B2/S34", gens))


def test_cli_refusals(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path, GOL_RULE="B3/S23VH")
    assert r.returncode != 0 and "'B3/S23VH'" in r.stderr
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path, GOL_RULE="B7/S2H")
    assert r.returncode != 0 and "'B7/S2H'" in r.stderr and "0 to 6" in r.stderr
    assert not list(tmp_path.glob("Rank_*"))  # a bad rule string ends the run before any rank started
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path, GOL_RULE=HEX, GOL_COMPAT="reference")
    assert r.returncode != 0 and HEX in r.stderr and "the reference has one rule, B3/S23" in r.stderr


def test_cli_pattern_file_sets_the_rule(gol_bin, tmp_path):
    rle = tmp_path / "p.rle"
    rle.write_text("x = 4, y = 4, rule = B2/S34H\n2o$4o$b2o$o!\n")
    r = _cli(gol_bin, [0, 64, 7, 64, 1], tmp_path / "a", GOL_PATTERN_FILE=rle, GOL_PATTERN_AT="30,30", GOL_RLE_OUT="final.rle")
    assert r.returncode == 0, r.stderr
    start = np.zeros((64, 64), np.uint8)
    start[30:34, 30:34] = np.array([[1, 1, 0, 0], [1, 1, 1, 1], [0, 1, 1, 0], [1, 0, 0, 0]], np.uint8)
    assert np.array_equal(_load(tmp_path / "a", 1), numpy_step_rule(start, HEX, 7))
    assert "rule = B2/S34H" in (tmp_path / "a" / "final.rle").read_text().splitlines()[0]
    r = _cli(gol_bin, [0, 64, 7, 64, 1], tmp_path / "b", GOL_PATTERN_FILE=rle, GOL_RULE="B2/S34")
    assert r.returncode != 0 and "B2/S34H" in r.stderr
    r = _cli(gol_bin, [0, 64, 7, 64, 1], tmp_path / "c", GOL_PATTERN_FILE=rle, GOL_RULE="s34/b2h")
    assert r.returncode == 0, r.stderr


# ----- checkpoints -----

def test_checkpoint_records_the_neighbourhood(gol, tmp_path):
    N, gens = 70, 9
    h = gol.Simulation(N, backend="cpu", rule=HEX).init(5, seed=4)
    h.step(gens)
    h.checkpoint(str(tmp_path / "h"))
    raw = (tmp_path / "h.gol").read_bytes()
    off = 8 + 6 * 8  # magic, then version, H, W, words_per_row, generation, seed
    code = int.from_bytes(raw[off : off + 8], "little")
    assert code == (1 << 2) | (2 << 12) | (((1 << 3) | (1 << 4)) << 16)
    again = gol.Simulation(N, backend="cpu", rule="s34/b2h").init(0)
    assert again.restore(str(tmp_path / "h")) == gens
    again.step(3)
    assert np.array_equal(again.board(), numpy_step_rule(initial_board(5, N, 1, True, 4), HEX, gens + 3))
    for other in ("B2/S34", "B2/S34V"):
        sim = gol.Simulation(N, backend="cpu", rule=other).init(0)
        with pytest.raises(gol.native.GolError) as e:
            sim.restore(str(tmp_path / "h"))
        assert HEX in str(e.value) and other in str(e.value)


def test_moore_checkpoint_format_is_unchanged(gol, tmp_path):
    """A Moore rule's code is the value written before there were neighbourhoods, and such a file restores."""
    N = 64
    d = gol.Simulation(N, backend="cpu").init(5, seed=4)
    d.checkpoint(str(tmp_path / "d"))
    raw = (tmp_path / "d.gol").read_bytes()
    off = 8 + 6 * 8
    assert int.from_bytes(raw[off : off + 8], "little") == 0x000C0008
    hl = gol.Simulation(N, backend="cpu", rule="B36/S23").init(5, seed=4)
    hl.checkpoint(str(tmp_path / "hl"))
    assert int.from_bytes((tmp_path / "hl.gol").read_bytes()[off : off + 8], "little") == 0x000C0048
    fresh = gol.Simulation(N, backend="cpu").init(0)
    fresh.restore(str(tmp_path / "d"))
    assert np.array_equal(fresh.board(), initial_board(5, N, 1, True, 4))
    hexsim = gol.Simulation(N, backend="cpu", rule="B3/S23H").init(0)
    with pytest.raises(gol.native.GolError):
        hexsim.restore(str(tmp_path / "d"))


def test_native_unit():
    r = subprocess.run([os.path.join(REPO, "build", "gol_nbhd_unit")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert ", 0 failed" in r.stdout
