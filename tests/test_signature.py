"""Signature mode (``signature=True``: the board signature and the population of every generation a run computes),
``signature()``, ``snapshot_diff()`` and ``find_cycle()`` on the CPU backend, the CLI and the Python API, against the
numpy oracles ``numpy_signature`` / ``numpy_signatures`` (which work from cells, not from packed words).

Every comparison is exact, and each also asserts that the final board is the oracle's, that the populations are
``numpy_census``'s, that the last signature is ``signature()`` and that the series holds at least two distinct
values.  Random boards keep the ghost rows and words live, so a hash that included a ghost cell would be wrong."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from cycle_cases import CYCLE_CASES, GLIDER_CELLS, GRID_CASES, brute_force_cycle, check_cycle, cycle_oracle
from gol_amd.ops import (
    Cycle,
    find_repeat,
    initial_board,
    numpy_census,
    numpy_signature,
    numpy_signatures,
    numpy_step_rule,
    numpy_step_rule_bounded,
    random_board,
)

RULES = ["B3/S23", "B36/S23", "B1357/S1357", "B1/S012345678"]
BOUNDARIES = ["torus", "dead"]
GLIDER = "x = 3, y = 3\nbob$2bo$3o!\n"
CPU_K = 4  # the CPU sweep's superstep depth: 2K + 1 = 9 generations


def one_cell(H, W, r, c):
    b = np.zeros((H, W), np.uint8)
    b[r, c] = 1
    return b


def test_vectors():
    """The seven published vectors."""
    assert numpy_signature(np.zeros((10, 70), np.uint8)) == 0
    assert numpy_signature(one_cell(8, 128, 0, 0)) == 0x0000000093257869
    assert numpy_signature(one_cell(8, 128, 0, 1)) == 0x00000000AAFB63CF
    assert numpy_signature(one_cell(8, 128, 1, 0)) == 0x0000000010C50FD7
    assert numpy_signature(one_cell(8, 128, 5, 63)) == 0x7956F7C180000000
    assert numpy_signature(one_cell(8, 128, 5, 64)) == 0x00000000EC8A0243
    b = np.zeros((200, 200), np.uint8)
    for r, c in GLIDER_CELLS:
        b[100 + r, 62 + c] = 1
    assert numpy_signature(b) == 0xE6FD2DE10676268A


def test_every_cell_has_its_own_signature():
    N = 137
    sigs = {numpy_signature(one_cell(N, N, r, c)) for r in range(N) for c in range(N)}
    assert len(sigs) == N * N and 0 not in sigs


def test_rectangle_swap_changes_the_signature():
    """Equal bits swapped between the corners of a rectangle of words: a sum of a row key and a column key would
    cancel identically; the product of the two does not."""
    a = np.zeros((10, 200), np.uint8)
    b = np.zeros((10, 200), np.uint8)
    a[2, 3] = a[7, 131] = 1
    b[2, 131] = b[7, 3] = 1
    assert numpy_signature(a) != numpy_signature(b)


def test_numpy_signatures_is_a_per_generation_loop():
    for bounded, step in [(False, numpy_step_rule), (True, numpy_step_rule_bounded)]:
        b = random_board(37, 70, 3)
        want = [numpy_signature(step(b, "B36/S23", g)) for g in range(1, 8)]
        got = numpy_signatures(b, "B36/S23", 7, bounded=bounded)
        assert got.dtype == np.uint64 and got.tolist() == want and len(set(want)) == 7
        sigs, last = numpy_signatures(b, "B36/S23", 7, bounded=bounded, return_board=True)
        assert np.array_equal(sigs, got) and np.array_equal(last, step(b, "B36/S23", 7))


@functools.lru_cache(maxsize=None)
def sweep_reference(N, rule, boundary, gens=2 * CPU_K + 1):
    b = initial_board(5, N, 1, True, N)
    sigs, board = numpy_signatures(b, rule, gens, bounded=boundary == "dead", return_board=True)
    return sigs, numpy_census(b, rule, gens, bounded=boundary == "dead"), board


def check(sim, start, sigs, pops, board, tiny=False):
    got_start, got, got_pops = sim.signatures()
    assert got_start == start and got.dtype == np.uint64 and got_pops.dtype == np.uint64
    assert np.array_equal(got, sigs), ([hex(v) for v in got.tolist()], [hex(v) for v in np.asarray(sigs).tolist()])
    assert np.array_equal(got_pops, pops), (got_pops.tolist(), np.asarray(pops).tolist())
    assert np.array_equal(sim.board(), board)
    assert int(got[-1]) == sim.signature() == numpy_signature(board)
    assert int(got_pops[-1]) == sim.population()
    assert tiny or len(set(got.tolist())) >= 2


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200])
def test_sweep(gol, N):
    gens = 2 * CPU_K + 1
    for boundary in BOUNDARIES:
        for rule in RULES:
            sigs, pops, board = sweep_reference(N, rule, boundary)
            s = gol.Simulation(N, backend="cpu", rule=rule, boundary=boundary, halo_depth=CPU_K, signature=True)
            s.init(5, seed=N).step(gens)
            assert s.stats()["signature"] is True and s.stats()["census"] is False
            check(s, 0, sigs, pops, board, tiny=N <= 3)


def _run_threads(gol, N, P, gens, backend="cpu", signature=True, **kw):
    ts = gol.parallel.thread_transports(P)
    out, errs = [None] * P, []

    def worker(r):
        try:
            s = gol.Simulation(N, ts[r], backend=backend, global_mode=True, signature=signature, **kw).init(5, seed=99)
            s.step(gens)
            rec = s.signatures() if signature else None
            out[r] = (s.geometry.row0, s.geometry.col0, s.board(), rec, s.signature(), s.population(), s.stats()["kernel"])
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


DECOMPOSITIONS = [(1, {}), (3, {}), (4, {"decomp": "2d", "grid": "2x2"}), (9, {"decomp": "2d", "grid": "3x3"})]


def test_signature_is_equal_across_decompositions(gol):
    """signature() of one board on P = 1, 3 strips, 2 x 2 and 3 x 3 thread ranks, without signature mode."""
    N, gens = 192, 5
    want = numpy_signature(numpy_step_rule(initial_board(5, N, 1, True, 99), "B3/S23", gens))
    for P, kw in DECOMPOSITIONS:
        _, out = _run_threads(gol, N, P, gens, signature=False, halo_depth=4, **kw)
        assert [o[4] for o in out] == [want] * P, (P, kw)


@pytest.mark.parametrize("P,kw", DECOMPOSITIONS[1:], ids=["P3", "2x2", "3x3"])
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_thread_ranks(gol, P, kw, boundary):
    """Every rank gets the same, global series; no rank hashes a ghost cell of its neighbour's."""
    N, gens, rule = 192, 11, "B36/S23"
    full, out = _run_threads(gol, N, P, gens, rule=rule, boundary=boundary, halo_depth=4, **kw)
    b0 = initial_board(5, N, 1, True, 99)
    sigs, board = numpy_signatures(b0, rule, gens, bounded=boundary == "dead", return_board=True)
    pops = numpy_census(b0, rule, gens, bounded=boundary == "dead")
    assert np.array_equal(full, board)
    for _, _, _, (start, got, got_pops), sig, pop, _ in out:
        assert start == 0 and np.array_equal(got, sigs) and np.array_equal(got_pops, pops)
        assert sig == int(sigs[-1]) and pop == int(pops[-1])
    assert len(set(sigs.tolist())) == gens


def test_several_steps_stamp_init_restore(gol, tmp_path):
    """One continuous series over several step() calls and a stamp(); init(), restore() and load_rle() clear it."""
    N, rule = 70, "B36/S23"
    s = gol.Simulation(N, backend="cpu", rule=rule, halo_depth=4, signature=True).init(5, seed=8)
    assert s.signatures()[0] == 0 and len(s.signatures()[1]) == 0 and len(s.signatures()[2]) == 0
    b0 = initial_board(5, N, 1, True, 8)
    assert s.signature() == numpy_signature(b0)
    s.step(5).step(20).step(1)
    s1, b = numpy_signatures(b0, rule, 26, return_board=True)
    p1 = numpy_census(b0, rule, 26)
    check(s, 0, s1, p1, b)
    s.stamp(GLIDER, at=(3, 3), mode="xor")  # the generation count runs on: so does the series
    b = s.board()
    assert s.signature() == numpy_signature(b)
    s.step(7)
    s2, b2 = numpy_signatures(b, rule, 7, return_board=True)
    p2 = numpy_census(b, rule, 7)
    check(s, 0, np.concatenate([s1, s2]), np.concatenate([p1, p2]), b2)
    s.checkpoint(str(tmp_path / "c"))
    s.signatures_clear()
    assert s.signatures()[0] == 33 and len(s.signatures()[1]) == 0
    s.step(3)
    s3, b3 = numpy_signatures(b2, rule, 3, return_board=True)
    p3 = numpy_census(b2, rule, 3)
    check(s, 33, s3, p3, b3)
    s.init(5, seed=8)
    assert s.signatures()[0] == 0 and len(s.signatures()[1]) == 0
    s.step(2)
    assert np.array_equal(s.signatures()[1], s1[:2])
    assert s.restore(str(tmp_path / "c")) == 33
    assert s.signatures()[0] == 33 and len(s.signatures()[1]) == 0
    s.step(3)
    check(s, 33, s3, p3, b3)
    s.load_rle(GLIDER)
    assert s.signatures()[0] == 0 and len(s.signatures()[1]) == 0
    s.step(4)
    assert s.signatures()[2].tolist() == [5, 5, 5, 5] and len(set(s.signatures()[1].tolist())) == 4


def test_snapshot_diff(gol):
    s = gol.Simulation(65, backend="cpu").init(5, seed=3)
    with pytest.raises(gol.native.GolError) as e:
        s.snapshot_diff()
    assert "snapshot" in str(e.value)
    s.snapshot()
    assert s.snapshot_diff() == 0
    s.stamp(np.ones((3, 3), np.uint8), at=(10, 20), mode="xor")
    assert s.snapshot_diff() == 9
    s.snapshot()
    s.stamp(np.ones((1, 1), np.uint8), at=(5, 64), mode="xor")  # the masked tail word of a 65-column board
    assert s.snapshot_diff() == 1


def test_rank_signature_mismatch_raises_everywhere(gol):
    P = 2
    ts = gol.parallel.thread_transports(P)
    errs = [None] * P

    def worker(r):
        try:
            gol.Simulation(64, ts[r], backend="cpu", signature=bool(r)).init(5, seed=1)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "signature" in str(e) and "disagree" in str(e) for e in errs), errs


def test_option_and_refusals(gol, monkeypatch):
    monkeypatch.delenv("GOL_SIGNATURE", raising=False)
    monkeypatch.delenv("GOL_CENSUS", raising=False)
    plain = gol.Simulation(16, backend="cpu").init(5)
    assert plain.stats()["signature"] is False and plain.config.signature is False
    for call in (plain.signatures, plain.signatures_clear, lambda: plain.find_cycle(10)):
        with pytest.raises(ValueError) as e:
            call()
        assert "signature=True" in str(e.value)
    with pytest.raises(gol.native.GolError) as e:  # the engine on its own
        plain.engine.signatures()
    assert "signature mode" in str(e.value)
    assert plain.signature() == numpy_signature(plain.board())  # any mode
    monkeypatch.setenv("GOL_SIGNATURE", "1")
    assert gol.Simulation(16, backend="cpu").stats()["signature"] is True
    assert gol.Simulation(16, backend="cpu", signature=False).stats()["signature"] is False
    monkeypatch.delenv("GOL_SIGNATURE")
    for kw, word in [({"census": True}, "census"), ({"compat": True}, "compat"), ({"subtiles": 2}, "subtiles=2")]:
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="cpu", signature=True, **kw)
        assert word in str(e.value) and "signature" in str(e.value)
    for kernel in ("temporal", "tile", "pipe", "resident", "lds"):
        with pytest.raises(ValueError) as e:
            gol.Simulation(64, backend="hip", signature=True, kernel=kernel)
        assert f"kernel {kernel!r} records no signatures" in str(e.value)
    D = gol.native.max_signature_depth()
    assert 4 <= D <= 8
    with pytest.raises(ValueError) as e:
        gol.Simulation(64, backend="hip", signature=True, kernel_depth=D + 1)
    assert f"deepest pass, {D} generations" in str(e.value)
    sim = gol.Simulation(64, backend="cpu")
    for field, value in [("compat", True), ("subtiles", 2), ("census", True)]:
        cfg = gol.native.EngineConfig()
        cfg.signature = True
        setattr(cfg, field, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(sim.geometry, cfg, sim.transport)
        assert "signature" in str(e.value)
    with pytest.raises(ValueError):
        gol.Simulation(16, backend="cpu", signature=True).init(5).find_cycle(0)


# ----- the pure cycle search -----

def test_find_repeat_collision_then_true_repeat():
    """A collision the verifier rejects is dropped; the true repeat after it is found."""
    series = [10, 11, 12, 11, 13, 14, 12, 99]  # generations 1 .. 8; 11 at 4 collides with 2, 12 at 7 is the repeat of 3
    calls = []

    def verify(g_prev, g):
        calls.append((g_prev, g))
        return (g_prev, g) == (3, 7)

    seen = {5: 0}
    assert find_repeat(series, seen, 1, verify) == (3, 7)
    assert calls == [(2, 4), (3, 7)]
    assert seen[11] == 2 and seen[13] == 5 and 99 not in seen  # the earlier generation keeps a hash; the search stopped at 7
    assert find_repeat([1, 2, 3], {}, 0, lambda a, b: True) is None
    assert find_repeat([7], {7: 0}, 1, lambda a, b: True) == (0, 1)
    assert find_repeat([7, 7], {7: 0}, 1, lambda a, b: False) is None
    # across chunks: `seen` carries over
    seen = {}
    assert find_repeat([1, 2, 3], seen, 0, lambda a, b: True) is None
    assert find_repeat([4, 2], seen, 3, lambda a, b: True) == (1, 4)
    assert Cycle(1, 3, 7, 5).period == 3


# ----- find_cycle -----

@pytest.mark.parametrize("name", list(CYCLE_CASES))
def test_find_cycle(gol, name):
    board, rule, boundary, max_generations, chunk = CYCLE_CASES[name]
    H, W = board.shape
    s = gol.Simulation(H, backend="cpu", width=W, rule=rule, boundary=boundary, halo_depth=8, signature=True).init(0)
    s.set_board(board)
    want = check_cycle(s, name, s.find_cycle(max_generations, chunk=chunk))
    assert np.array_equal(s.board(), want)
    if name == "dies-out":
        assert s.population() == 0 and cycle_oracle(name)[1] == 1


def test_find_cycle_budget_ends_first(gol):
    board = CYCLE_CASES["rpent-64"][0]
    assert brute_force_cycle(board, "B3/S23", False, 100) is None
    s = gol.Simulation(64, backend="cpu", halo_depth=8, signature=True).init(0)
    s.set_board(board)
    assert s.find_cycle(100, chunk=32) is None
    assert s.generation == 100 and np.array_equal(s.board(), numpy_step_rule(board, "B3/S23", 100))


@pytest.mark.parametrize("name", GRID_CASES)
def test_find_cycle_thread_ranks(gol, name):
    """Collective: every rank of a 2 x 2 grid returns the same record."""
    board, rule, boundary, max_generations, chunk = CYCLE_CASES[name]
    H, W = board.shape
    P = 4
    ts = gol.parallel.thread_transports(P)
    out, errs = [None] * P, []

    def worker(r):
        try:
            s = gol.Simulation(H, ts[r], backend="cpu", global_mode=True, width=W, decomp="2d", grid="2x2", halo_depth=8,
                               rule=rule, boundary=boundary, signature=True).init(0)
            s.stamp(board, at=(0, 0), mode="or")
            out[r] = s.find_cycle(max_generations, chunk=chunk)
        except Exception as e:
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    transient, period, _ = cycle_oracle(name)
    assert all(o == out[0] for o in out) and (out[0].transient, out[0].period) == (transient, period)


# ----- CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "cpu"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_BOUNDARY",
              "GOL_PATTERN_FILE", "GOL_PATTERN_AT", "GOL_RLE_OUT", "GOL_CENSUS", "GOL_CENSUS_OUT", "GOL_COMPAT", "GOL_SUBTILES",
              "GOL_SIGNATURE", "GOL_SIGNATURE_OUT"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_cli_signature_out(gol_bin, tmp_path, P, boundary):
    N, gens, rule = 48, 13, "B36/S23"
    r = _cli(gol_bin, [5, N, gens, 64, 0], tmp_path, GOL_SIGNATURE_OUT=tmp_path / "sig.csv", GOL_NRANKS=P, GOL_RULE=rule,
             GOL_BOUNDARY=boundary, GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    lines = (tmp_path / "sig.csv").read_text().splitlines()
    assert lines[0] == "generation,population,signature"
    rows = [ln.split(",") for ln in lines[1:]]
    b0 = initial_board(5, N, P, True)
    sigs = numpy_signatures(b0, rule, gens, bounded=boundary == "dead")
    pops = numpy_census(b0, rule, gens, bounded=boundary == "dead")
    assert [int(a) for a, _, _ in rows] == list(range(1, gens + 1))
    assert [int(p) for _, p, _ in rows] == pops.tolist()
    assert [s for _, _, s in rows] == ["%016x" % v for v in sigs.tolist()] and len(set(sigs.tolist())) == gens
    assert '"signature": true' in (tmp_path / "m.json").read_text()


def test_cli_signature_flag_alone_and_default(gol_bin, tmp_path):
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "a", GOL_SIGNATURE=1, GOL_METRICS_JSON=tmp_path / "a" / "m.json")
    assert r.returncode == 0, r.stderr
    assert '"signature": true' in (tmp_path / "a" / "m.json").read_text()
    r = _cli(gol_bin, [5, 64, 6, 64, 0], tmp_path / "b", GOL_METRICS_JSON=tmp_path / "b" / "m.json")
    assert r.returncode == 0, r.stderr
    assert '"signature": false' in (tmp_path / "b" / "m.json").read_text()


@pytest.mark.parametrize("P", [1, 3])
def test_cli_unwritable_path(gol_bin, tmp_path, P):
    bad = tmp_path / "no" / "such" / "dir" / "sig.csv"
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_SIGNATURE_OUT=bad, GOL_NRANKS=P)
    assert r.returncode != 0 and str(bad) in r.stderr and "GOL_SIGNATURE_OUT" in r.stderr


@pytest.mark.parametrize("env", [{"GOL_COMPAT": "reference"}, {"GOL_SUBTILES": 2}, {"GOL_CENSUS": 1}],
                         ids=["compat", "subtiles", "census"])
def test_cli_refusals(gol_bin, tmp_path, env):
    r = _cli(gol_bin, [5, 48, 5, 64, 0], tmp_path, GOL_SIGNATURE=1, **env)
    assert r.returncode != 0 and "signature" in r.stderr
