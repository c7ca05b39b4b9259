"""Life-like rules (B.../S... strings) on the CPU backend, the CLI and the Python API, against the
byte-per-cell numpy oracle ``numpy_step_rule`` (which parses rules on its own)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from gol_amd.ops import initial_board, numpy_step, numpy_step_rule, parse_rule, rule_string
from gol_amd.utils import read_dump

NAMED = {
    "HighLife": "B36/S23",
    "Day & Night": "B3678/S34678",
    "Seeds": "B2/S",
    "Replicator": "B1357/S1357",
    "Life without death": "B3/S012345678",
    "Diamoeba": "B35678/S5678",
}
SINGLE_BIT = [f"B{c}/S" for c in range(1, 9)] + [f"B/S{c}" for c in range(9)]


def random_rules(n=8):
    rng = np.random.default_rng(0)
    out = []
    for _ in range(n):
        birth, survive = (int(v) for v in rng.integers(0, 512, size=2))
        out.append(rule_string((birth & ~1, survive)))
    return out


def neighbour_pairs(board):
    """How often each (state, live-neighbour count) pair occurs on the torus: array [2, 9]."""
    b = board.astype(np.int64)
    n = sum(np.roll(np.roll(b, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
    return np.array([[int(((b == s) & (n == c)).sum()) for c in range(9)] for s in (0, 1)])


@pytest.fixture(scope="module")
def board128():
    return initial_board(5, 128, 1, True, 1)


def test_board_covers_every_pair(board128):
    """The single-bit tests below exercise every entry of the rule table: pattern 5, N = 128, seed 1 holds
    each of the 18 (state, count) pairs at least 25 times."""
    assert neighbour_pairs(board128).min() >= 25, neighbour_pairs(board128)


@pytest.mark.parametrize("rule", SINGLE_BIT)
def test_single_bit_rules(gol, board128, rule):
    assert neighbour_pairs(board128).min() >= 25
    s = gol.Simulation(128, backend="cpu", rule=rule).init(5, seed=1)
    s.step(1)
    assert np.array_equal(s.board(), numpy_step_rule(board128, rule, 1))


def test_oracle_is_conway_for_b3s23():
    b = initial_board(5, 65, 1, True, 3)
    assert np.array_equal(numpy_step_rule(b, "B3/S23", 5), numpy_step(b, 5))
    assert np.array_equal(numpy_step_rule(b, (1 << 3, (1 << 2) | (1 << 3)), 5), numpy_step(b, 5))


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 137])
@pytest.mark.parametrize("rule", list(NAMED.values()) + random_rules())
def test_rules_vs_numpy(gol, rule, N):
    gens = 11
    s = gol.Simulation(N, backend="cpu", rule=rule).init(5, seed=7)
    s.step(gens)
    assert s.stats()["rule"] == rule
    assert np.array_equal(s.board(), numpy_step_rule(initial_board(5, N, 1, True, 7), rule, gens))


def _run_threads(gol, N, P, gens, **kw):
    ts = gol.parallel.thread_transports(P)
    boards, errs = [None] * P, []

    def worker(r):
        try:
            s = gol.Simulation(N, ts[r], backend="cpu", **kw).init(5, seed=99)
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


@pytest.mark.parametrize("P,kw", [(2, {}), (3, {}), (4, {"decomp": "2d", "grid": "2x2", "global_mode": True})])
def test_highlife_thread_ranks(gol, P, kw):
    N, gens = 96, 19
    full = _run_threads(gol, N, P, gens, rule="B36/S23", halo_depth=4, **kw)
    per_rank = not kw.get("global_mode", False)
    assert np.array_equal(full, numpy_step_rule(initial_board(5, N, P, per_rank, 99), "B36/S23", gens))


def test_rank_rule_mismatch_raises_everywhere(gol):
    """Ranks that disagree on the rule all raise at init; none hangs."""
    P = 2
    ts = gol.parallel.thread_transports(P)
    errs = [None] * P

    def worker(r):
        try:
            gol.Simulation(64, ts[r], backend="cpu", rule=["B36/S23", "B3/S23"][r]).init(5, seed=1)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "rule" in str(e) for e in errs), errs


# ----- CLI -----

def _cli(gol_bin, args, cwd, rule=None):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS"):
        e.pop(k, None)
    if rule is not None:
        e["GOL_RULE"] = rule
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


def test_cli_highlife_dump(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path, "B36/S23")
    assert r.returncode == 0, r.stderr
    rank, first, cells = read_dump(os.path.join(tmp_path, "Rank_0_of_1.txt"))
    assert np.array_equal(cells, numpy_step_rule(initial_board(5, 64), "B36/S23", 10))
    assert not np.array_equal(cells, numpy_step(initial_board(5, 64), 10))  # (the rule does matter on this board)


def test_cli_default_rule_unchanged(gol_bin, tmp_path):
    """GOL_RULE unset and GOL_RULE=B3/S23: the same stdout (but for the measured duration, a wall-clock
    figure) and byte-identical dumps, equal to the B3/S23 oracle."""
    outs, dumps = [], []
    for i, rule in enumerate([None, "B3/S23"]):
        cwd = tmp_path / str(i)
        r = _cli(gol_bin, [5, 64, 10, 64, 1], cwd, rule)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        outs.append(re.sub(r"TOTAL DURATION : \S+", "TOTAL DURATION : T", r.stdout))
        dumps.append((cwd / "Rank_0_of_1.txt").read_bytes())
    assert outs[0] == outs[1] and outs[0].startswith("TOTAL DURATION : T")
    assert dumps[0] == dumps[1]
    _, _, cells = read_dump(os.path.join(tmp_path, "0", "Rank_0_of_1.txt"))
    assert np.array_equal(cells, numpy_step(initial_board(5, 64), 10))


def test_cli_b0_rejected(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 10, 64, 1], tmp_path, "B0/S")
    assert r.returncode != 0
    assert "'B0/S'" in r.stderr and "B0" in r.stderr and "out of scope" in r.stderr
    assert not list(tmp_path.glob("Rank_*"))  # before any rank started


# ----- Python API -----

def test_stats_rule_is_canonical(gol):
    assert gol.Simulation(16, backend="cpu").stats()["rule"] == "B3/S23"
    assert gol.Simulation(16, backend="cpu", rule="s23/b3").init(5).stats()["rule"] == "B3/S23"
    assert gol.Simulation(16, backend="cpu", rule="b63/s32").stats()["rule"] == "B36/S23"
    assert "rule B36/S23" in gol.Simulation(16, backend="cpu", rule="highlife").describe()


@pytest.mark.parametrize("alias,rule", [("conway", "B3/S23"), ("life", "B3/S23"), ("highlife", "B36/S23"),
                                        ("daynight", "B3678/S34678"), ("seeds", "B2/S"), ("replicator", "B1357/S1357")])
def test_aliases(gol, alias, rule):
    assert gol.Simulation(16, backend="cpu", rule=alias).stats()["rule"] == rule
    assert gol.native.parse_rule(alias) == parse_rule(rule) == parse_rule(alias)


@pytest.mark.parametrize("rule", list(NAMED.values()) + random_rules() + SINGLE_BIT)
def test_native_and_python_parsers_agree(gol, rule):
    assert tuple(gol.native.parse_rule(rule)) == parse_rule(rule)
    assert rule_string(parse_rule(rule)) == rule


@pytest.mark.parametrize("bad", ["B39/S23", "B33/S23", "B3", "S23", "B3/S23x", "B0/S", "B03/S23", "", "B3/B3"])
def test_bad_rules_raise_value_error(gol, bad):
    with pytest.raises(ValueError) as e:
        gol.native.parse_rule(bad)
    assert f"'{bad}'" in str(e.value)
    with pytest.raises(ValueError):
        gol.Simulation(16, backend="cpu", rule=bad)
    with pytest.raises(ValueError):
        parse_rule(bad)


def test_checkpoint_rule(gol, tmp_path):
    N, gens = 70, 9
    hl = gol.Simulation(N, backend="cpu", rule="B36/S23").init(5, seed=4)
    hl.step(gens)
    hl.checkpoint(str(tmp_path / "hl"))
    again = gol.Simulation(N, backend="cpu", rule="highlife").init(0)
    assert again.restore(str(tmp_path / "hl")) == gens
    again.step(3)
    assert np.array_equal(again.board(), numpy_step_rule(initial_board(5, N, 1, True, 4), "B36/S23", gens + 3))
    conway = gol.Simulation(N, backend="cpu").init(0)
    with pytest.raises(gol.native.GolError) as e:
        conway.restore(str(tmp_path / "hl"))
    assert "B36/S23" in str(e.value) and "B3/S23" in str(e.value)
    # a default Simulation's file restores under the default, and not under another rule
    d = gol.Simulation(N, backend="cpu").init(5, seed=4)
    d.step(gens)
    d.checkpoint(str(tmp_path / "d"))
    assert conway.restore(str(tmp_path / "d")) == gens
    assert np.array_equal(conway.board(), numpy_step(initial_board(5, N, 1, True, 4), gens))
    with pytest.raises(gol.native.GolError):
        again.restore(str(tmp_path / "d"))


def test_old_checkpoint_without_rule_field_loads(gol, tmp_path):
    """Files written before the rule was stored have 0 in the header's reserved word: B3/S23."""
    N = 64
    d = gol.Simulation(N, backend="cpu").init(5, seed=4)
    d.checkpoint(str(tmp_path / "old"))
    p = tmp_path / "old.gol"
    raw = bytearray(p.read_bytes())
    off = 8 + 6 * 8  # magic, then version, H, W, words_per_row, generation, seed
    assert int.from_bytes(raw[off : off + 8], "little") == (1 << 3) | (((1 << 2) | (1 << 3)) << 16)
    raw[off : off + 8] = bytes(8)
    p.write_bytes(bytes(raw))
    fresh = gol.Simulation(N, backend="cpu").init(0)
    fresh.restore(str(tmp_path / "old"))
    assert np.array_equal(fresh.board(), initial_board(5, N, 1, True, 4))


def test_restrictions(gol):
    with pytest.raises((ValueError, RuntimeError)):
        gol.Simulation(64, backend="cpu", rule="B36/S23", compat=True)
    with pytest.raises((ValueError, RuntimeError)):
        gol.Simulation(64, backend="cpu", rule="B36/S23", subtiles=2)
    gol.Simulation(64, backend="cpu", rule="B3/S23", compat=True)  # the default rule keeps compat mode
    # the native engine refuses them on its own as well
    cfg = gol.native.EngineConfig()
    cfg.rule = "B36/S23"
    cfg.compat = True
    sim = gol.Simulation(64, backend="cpu")
    with pytest.raises(gol.native.GolError):
        gol.native.Engine.create(sim.geometry, cfg, sim.transport)
