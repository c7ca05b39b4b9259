"""Larger than Life rules (R<r>,C<c>,M<m>,S<a>..<b>,B<a>..<b>[,NM]) without a GPU: the rule strings against the Python
parser, the numpy oracle against the life-like oracles at range 1, the CPU backend against ``numpy_ltl`` over the cases
of ltl_cases.py (every range, an M1 and an M0 rule, tail and wrap shapes, both boundaries), the board's readers and
writers, RLE files, and everything this version refuses with such a rule.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import ltl_cases as lc
from gol_amd.ops import (numpy_ltl, numpy_step_rule, numpy_step_rule_bounded, parse_ltl_rule, parse_rule_states, random_board)

BOSCO = "R5,C0,M1,S34..58,B34..45,NM"


def _sim(gol, N, **kw):
    kw.setdefault("backend", "cpu")
    return gol.Simulation(N, **kw)


# ----- the rule strings -----

ACCEPTED = [
    (BOSCO, BOSCO, (5, 1, 34, 58, 34, 45)),
    ("bosco", BOSCO, (5, 1, 34, 58, 34, 45)),
    ("Bosco", BOSCO, (5, 1, 34, 58, 34, 45)),
    ("r5,c0,m1,s34..58,b34..45,nm", BOSCO, (5, 1, 34, 58, 34, 45)),
    ("R5,C0,M1,S34..58,B34..45", BOSCO, (5, 1, 34, 58, 34, 45)),
    ("R5,C2,M1,S34..58,B34..45,NM", BOSCO, (5, 1, 34, 58, 34, 45)),
    ("R1,C0,M0,S2..3,B3..3,NM", "R1,C0,M0,S2..3,B3..3,NM", (1, 0, 2, 3, 3, 3)),
    ("r7,c0,m1,s63..108,b63..84", "R7,C0,M1,S63..108,B63..84,NM", (7, 1, 63, 108, 63, 84)),
    ("R7,C0,M0,S0..225,B1..225,NM", "R7,C0,M0,S0..225,B1..225,NM", (7, 0, 0, 225, 1, 225)),
    ("R2,C0,M1,S0..0,B25..25", "R2,C0,M1,S0..0,B25..25,NM", (2, 1, 0, 0, 25, 25)),
]

REJECTED = [
    ("R0,C0,M1,S1..1,B1..1,NM", "R1 to R7"), ("R8,C0,M1,S34..58,B34..45,NM", "R1 to R7"), ("R12,C0,M1,S34..58,B34..45,NM", "R1 to R7"),
    ("R5,C3,M1,S34..58,B34..45,NM", "not built"), ("R5,C4,M1,S34..58,B34..45,NM", "history states"),
    ("R5,C1,M1,S34..58,B34..45,NM", "C1"), ("R5,C0,M2,S34..58,B34..45,NM", "M2"),
    ("R5,C0,M1,S34..58,B34..45,NN", "NN"), ("R5,C0,M1,S34..58,B34..45,NC", "NC"), ("R5,C0,M1,S34..58,B34..45,NX", "NM"),
    ("R5,C0,M1,S58..34,B34..45,NM", "min <= max"), ("R5,C0,M1,S34..122,B34..45,NM", "121"),
    ("R5,C0,M1,S34..58,B45..34,NM", "min <= max"), ("R5,C0,M1,S34..58,B34..122,NM", "121"),
    ("R1,C0,M0,S2..3,B3..10,NM", "= 9"),
    ("R5,C0,M1,S34..58,B0..45,NM", "B0 rules are out of scope"), ("R5,C0,M1,S34..58,B0..0,NM", "B0 rules are out of scope"),
    ("R5,R5,C0,M1,S34..58,B34..45,NM", "twice"), ("R5,C0,M1,S34..58,B34..45,B34..45,NM", "twice"),
    ("R5,C0,M1,S34..58,B34..45,NM,NM", "twice"),
    ("R5,M1,S34..58,B34..45,NM", "missing"), ("R5,C0,S34..58,B34..45,NM", "missing"), ("R5,C0,M1,B34..45,NM", "missing"),
    ("R5,C0,M1,S34..58,NM", "missing"),
    ("R5,C0,M1,S34..58,B34..45,NM,", "trailing comma"), ("R5,C0,M1,S34..58,B34..45,", "trailing comma"),
    ("R5, C0,M1,S34..58,B34..45,NM", "spaces"), ("R5,C0,M1,S34..58,B34..45,NM ", "spaces"), (" R5,C0,M1,S34..58,B34..45,NM", None),
    ("R05,C0,M1,S34..58,B34..45,NM", "leading zero"), ("R5,C00,M1,S34..58,B34..45,NM", "leading zero"),
    ("R5,C0,M01,S34..58,B34..45,NM", "leading zero"), ("R5,C0,M1,S034..58,B34..45,NM", "leading zero"),
    ("R5,C0,M1,S34..058,B34..45,NM", "leading zero"), ("R5,C0,M1,S34..58,B034..45,NM", "leading zero"),
    ("R5,C0,M1,S34-58,B34..45,NM", None), ("R5,C0,M1,S34..,B34..45,NM", None), ("R5,C0,M1,S..58,B34..45,NM", None),
    ("R5,C0,M1,S34...58,B34..45,NM", None), ("R,C0,M1,S34..58,B34..45,NM", None), ("R5,,C0,M1,S34..58,B34..45,NM", None),
    ("R5,C0,M1,B34..45,S34..58,NM", "order"), ("R5,C0,M1,S34..58,B34..45,NM,X1", None), ("R5,C0,M1,S34..58,B34..45,NM/C3", None),
    ("R5", None), ("R5,C0,M1,S34..58,B34..45,N", None), ("bosco2", None),
]


@pytest.mark.parametrize("text,canonical,fields", ACCEPTED)
def test_rule_accepted(gol, text, canonical, fields):
    """The native parser, the Python parser and the canonical form agree."""
    assert parse_ltl_rule(text) == fields
    assert tuple(gol.native.parse_ltl_rule(text)) == fields
    assert gol.native.canonical_rule(text) == canonical == gol.ops.ltl_rule_string(text)
    assert parse_rule_states(text) == 2 == gol.native.parse_rule_states(text)
    cfg = gol.native.EngineConfig()
    cfg.rule = text
    assert cfg.rule == canonical


@pytest.mark.parametrize("text,word", REJECTED, ids=[t for t, _ in REJECTED])
def test_rule_rejected(gol, text, word):
    """Both parsers refuse the string as an invalid rule, and name it."""
    with pytest.raises(ValueError, match="invalid rule") as e:
        gol.native.parse_ltl_rule(text)
    assert repr(text)[1:-1] in str(e.value) or text in str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="invalid rule"):
        parse_ltl_rule(text)
    with pytest.raises(ValueError, match="invalid rule"):
        gol.Simulation(64, rule=text, backend="cpu")


def test_b0_wording_is_the_parsers(gol):
    """bmin = 0 is the B0 case, refused in the words the parser uses for B0 rules."""
    def message(rule):
        with pytest.raises(ValueError) as e:
            gol.native.parse_rule(rule)
        return str(e.value).split(": ", 1)[1]

    assert message("R5,C0,M1,S34..58,B0..45,NM") == message("B03/S23")


def test_existing_rules_keep_their_results(gol):
    assert gol.native.parse_ltl_rule("B3/S23") is None and gol.native.parse_ltl_rule("replicator") is None
    assert gol.native.parse_ltl_rule("B2/S345/C4") is None
    assert gol.native.parse_rule("replicator") == gol.native.parse_rule("B1357/S1357")
    assert gol.native.canonical_rule("s23/b3") == "B3/S23" and gol.native.canonical_rule("345/2/4") == "B2/S345/C4"
    assert not gol.ops.is_ltl_rule("replicator") and gol.ops.is_ltl_rule("bosco") and gol.ops.is_ltl_rule("r1,c0")


def test_thresholds(gol):
    """The folding of M into thresholds on the sum that includes the centre, with the clamps."""
    assert gol.native.ltl_thresholds("bosco") == (34, 45, 34, 58)
    assert gol.native.ltl_thresholds("R5,C0,M0,S33..57,B34..45") == (34, 45, 34, 58)
    assert gol.native.ltl_thresholds("R1,C0,M0,S2..3,B3..3") == (3, 3, 3, 4)
    assert gol.native.ltl_thresholds("R1,C0,M0,S2..9,B3..9") == (3, 9, 3, 9)
    blo, bhi, slo, shi = gol.native.ltl_thresholds("R1,C0,M0,S9..9,B3..3")  # nine neighbours beside the centre: never
    assert slo > shi and max(blo, bhi, slo, shi) <= 9
    with pytest.raises(ValueError, match="B3/S23"):
        gol.native.ltl_thresholds("B3/S23")


# ----- the oracle -----

@pytest.mark.parametrize("rule", ["R1,C0,M0,S2..3,B3..3,NM", "R1,C0,M1,S3..4,B3..3,NM"])
def test_oracle_is_life_at_range_one(rule):
    """Both spellings of B3/S23 as a range-1 rule, over 8 generations, on the torus and on a bounded board."""
    b = random_board(37, 70, 11)
    t, d = b, b
    for g in range(1, 9):
        t, d = numpy_ltl(t, rule, 1), numpy_ltl(d, rule, 1, boundary="dead")
        assert np.array_equal(t, numpy_step_rule(b, "B3/S23", g))
        assert np.array_equal(d, numpy_step_rule_bounded(b, "B3/S23", g))
    assert t.any() and not np.array_equal(t, d)
    assert np.array_equal(numpy_ltl(b, rule, 8), t)


def test_oracle_by_hand():
    """Counts by hand: a 3 x 3 block under a range-2 rule, with and without the middle cell."""
    b = np.zeros((9, 9), np.uint8)
    b[3:6, 3:6] = 1
    # every cell of the block sees all nine (M1) or eight (M0); the cell at (2, 2) sees four, its box is rows 0..4
    assert np.array_equal(numpy_ltl(b, "R2,C0,M1,S9..9,B4..4", 1)[3:6, 3:6], np.ones((3, 3), np.uint8))
    assert numpy_ltl(b, "R2,C0,M1,S9..9,B4..4", 1)[2, 2] == 1 and numpy_ltl(b, "R2,C0,M1,S9..9,B5..5", 1)[2, 2] == 0
    assert not numpy_ltl(b, "R2,C0,M0,S9..9,B25..25", 1).any()
    assert np.array_equal(numpy_ltl(b, "R2,C0,M0,S8..8,B25..25", 1), b)
    # a bounded board: the corner cell of a full 5 x 5 board sees 9 cells under range 2, on the torus all 25
    full = np.ones((5, 5), np.uint8)
    assert numpy_ltl(full, "R2,C0,M1,S9..9,B1..1", 1, boundary="dead")[0, 0] == 1
    assert numpy_ltl(full, "R2,C0,M1,S9..9,B1..1", 1)[0, 0] == 0
    with pytest.raises(ValueError, match="smaller"):
        numpy_ltl(np.zeros((4, 9), np.uint8), "R2,C0,M1,S9..9,B1..1", 1)


# ----- the CPU backend -----

@pytest.mark.parametrize("boundary", lc.BOUNDARIES)
@pytest.mark.parametrize("R", lc.RANGES)
def test_cpu_engine(gol, R, boundary):
    """Every shape of the range under both rules: two generations, compared after each."""
    for rule in lc.rules(R):
        for H, W in lc.shapes(R):
            lc.run_case(lambda n, **kw: _sim(gol, n, **kw), rule, H, W, boundary, kernel="cpu")


def test_cpu_engine_keeps_changing(gol):
    """Three generations at 137 x 137, where every rule keeps changing."""
    for R in lc.RANGES:
        for rule in lc.rules(R):
            seed = lc.seed_of(137, 137, rule, "torus")
            assert lc.lively(137, 137, seed, rule, "torus", 3)
            h = lc.history(137, 137, seed, rule, "torus", 3)
            s = lc.start_sim(_sim(gol, 137, rule=rule), 137, 137, seed)
            s.step(3)
            lc.check(s, h[3], "cpu")


def test_life_through_the_ltl_stepper(gol):
    """B3/S23 as a range-1 rule against the life-like stepper: boards, fingerprints and signatures over 17 generations."""
    start = random_board(137, 137, 3)
    for boundary in lc.BOUNDARIES:
        a = _sim(gol, 137, rule="R1,C0,M0,S2..3,B3..3,NM", boundary=boundary)
        b = _sim(gol, 137, rule="B3/S23", boundary=boundary)
        for s in (a, b):
            s.init(0)
            s.set_board(start)
            s.step(17)
        assert np.array_equal(a.board(), b.board()) and a.board().any()
        assert a.fingerprint() == b.fingerprint() and a.signature() == b.signature()


@pytest.mark.parametrize("boundary", lc.BOUNDARIES)
def test_stamp_and_window_across_the_seams(gol, boundary):
    H, W, rule = 65, 137, BOSCO
    seed = lc.seed_of(H, W, rule, boundary)
    b0 = lc.start_board(H, W, seed)
    s = lc.start_sim(_sim(gol, H, width=W, rule=rule, boundary=boundary), H, W, seed)
    s.step(1)
    b1 = numpy_ltl(b0, rule, 1, boundary=boundary)
    pat = random_board(20, 90, 5)
    at = (55, 100) if boundary == "torus" else (40, 40)  # (the torus: across both seams)
    s.stamp(pat, at=at, mode="or")
    want = b1.copy()
    rr, cc = np.ix_(np.arange(at[0], at[0] + 20) % H, np.arange(at[1], at[1] + 90) % W)
    want[rr, cc] |= pat
    lc.check(s, want)
    if boundary == "torus":
        win = s.window(60, 130, 12, 20)
        assert np.array_equal(win, want[np.ix_(np.arange(60, 72) % H, np.arange(130, 150) % W)])
    else:
        assert np.array_equal(s.window(50, 100, 12, 20), want[50:62, 100:120])
    s.step(2)
    lc.check(s, numpy_ltl(want, rule, 2, boundary=boundary))
    assert s.generation == 3


def test_board_readers(gol):
    """density, match, count_matches, signature, snapshot and population on an LtL simulation read the ordinary board."""
    H, W, rule = 64, 128, BOSCO
    seed = lc.seed_of(H, W, rule, "torus")
    s = lc.start_sim(_sim(gol, H, width=W, rule=rule), H, W, seed)
    s.step(2)
    ref = numpy_ltl(lc.start_board(H, W, seed), rule, 2)
    p = _sim(gol, H, width=W)  # a life-like simulation holding the same cells
    p.init(0)
    p.set_board(ref)
    assert s.population() == p.population() == int(ref.sum())
    assert s.fingerprint() == p.fingerprint() and s.signature() == p.signature()
    assert np.array_equal(s.density(16, 64), p.density(16, 64))
    block = np.ones((2, 2), np.uint8)
    assert s.count_matches(block, margin=0) == p.count_matches(block, margin=0) > 0
    s.snapshot()
    assert s.snapshot_diff() == 0
    s.step(1)
    assert s.snapshot_diff() == int((numpy_ltl(ref, rule, 1) != ref).sum()) > 0


def test_rle_round_trip(gol, tmp_path):
    """from_rle of a file whose header names an LtL rule, with and without a topology suffix; save_rle writes it back."""
    H, W = 40, 70
    cells = lc.start_board(H, W, 5)
    for suffix, boundary in (("", "torus"), (f":T{W},{H}", "torus"), (f":P{W},{H}", "dead")):
        path = tmp_path / f"b{len(suffix)}{boundary}.rle"
        path.write_text(gol.ops.write_rle(cells, BOSCO).replace(f"rule = {BOSCO}", f"rule = {BOSCO}{suffix}"))
        assert f"rule = {BOSCO}{suffix}\n" in path.read_text()
        s = gol.Simulation.from_rle(str(path), None if suffix else H, backend="cpu", **({} if suffix else {"width": W}))
        assert s.config.rule == BOSCO and s.config.boundary == boundary and s.ltl == (5, 1, 34, 58, 34, 45)
        lc.check(s, cells, "cpu")
        s.step(2)
        lc.check(s, numpy_ltl(cells, BOSCO, 2, boundary=boundary))
        out = tmp_path / f"out{len(suffix)}{boundary}.rle"
        s.save_rle(str(out))
        back, rule = gol.ops.parse_rle(out.read_text())
        assert rule == BOSCO and np.array_equal(back, numpy_ltl(cells, BOSCO, 2, boundary=boundary)[: back.shape[0], : back.shape[1]])
        assert (f"rule = {BOSCO}:P{W},{H}" in out.read_text()) == (boundary == "dead")
    with pytest.raises(ValueError, match="names rule R5"):
        gol.Simulation.from_rle(str(path), backend="cpu", rule="R5,C0,M0,S34..58,B34..45")
    # the lower-case header Golly may write, and the alias
    text = "x = 3, y = 1, rule = r5,c0,m1,s34..58,b34..45,nm\n3o!\n"
    assert gol.ops.parse_rle(text)[1] == BOSCO


def test_board_size_error(gol):
    for kw in ({"width": 64}, {"width": 10}):
        N = 10 if kw["width"] == 64 else 64
        with pytest.raises(ValueError, match="11 x 11") as e:
            _sim(gol, N, rule=BOSCO, **kw)
        assert BOSCO in str(e.value) and f"{N} x {kw['width']}" in str(e.value)
    geo = gol.native.make_geometry(gol.native.make_decomposition(10, 1, False, "1d", "", 64), 0)
    cfg = gol.native.EngineConfig()
    cfg.backend = "cpu"
    cfg.rule = BOSCO
    with pytest.raises(gol.native.GolError, match="11 x 11") as e:
        gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
    assert BOSCO in str(e.value) and "10 x 64" in str(e.value)
    _sim(gol, 11, rule=BOSCO, width=11).init(5, seed=1).step(1)  # the smallest board runs


# ----- refusals -----

REFUSED = [
    ({"census": True}, "census"), ({"signature": True}, "signature"), ({"film": (0, 0, 8, 8)}, "film"),
    ({"density_film": (8, 64)}, "density_film"), ({"envelope": True}, "envelope"), ({"compat": True}, "compat"),
    ({"subtiles": 2}, "subtiles"), ({"self_exchange": True}, "self_exchange"), ({"force_split": True}, "force_split"),
    ({"backend": "hip", "kernel": "temporal"}, "temporal"), ({"backend": "hip", "kernel": "tile"}, "tile"),
    ({"backend": "hip", "kernel": "pipe"}, "pipe"), ({"backend": "hip", "kernel": "resident"}, "resident"),
    ({"backend": "hip", "kernel": "lds"}, "lds"), ({"kernel_depth": 2}, "kernel_depth 2"), ({"kernel_depth": 8}, "kernel_depth 8"),
    ({"halo_depth": 2}, "halo_depth 2"), ({"halo_depth": 32}, "halo_depth 32"),
]


@pytest.mark.parametrize("kw,names", REFUSED, ids=[n for _, n in REFUSED])
def test_constructor_refusals(gol, kw, names):
    kw = dict(kw)
    kw.setdefault("backend", "cpu")
    with pytest.raises(ValueError, match=names) as e:
        gol.Simulation(64, rule=BOSCO, **kw)
    assert BOSCO in str(e.value)


def test_depth_one_is_accepted(gol):
    s = _sim(gol, 64, rule=BOSCO, kernel_depth=1, halo_depth=1).init(5, seed=1)
    s.step(2)
    st = s.stats()
    assert st["depth"] == 1 and st["kernel_depth"] == 1 and st["states"] == 2 and st["rule"] == BOSCO and s.generation == 2


def test_engine_refusals(gol):
    """The engine's own constructor refuses what the Python one does, each error naming the option and the rule."""
    geo = gol.native.make_geometry(gol.native.make_decomposition(64, 1, False, "1d", "", 0), 0)
    for field, value, names in [("census", True, "census"), ("signature", True, "signature"), ("film", (0, 0, 8, 8), "film"),
                                ("density_film", (8, 64), "density_film"), ("envelope", True, "envelope"),
                                ("compat", True, "compat"), ("subtiles", 2, "subtiles"), ("self_exchange", True, "self_exchange"),
                                ("force_split", True, "force_split"), ("kernel_depth", 3, "kernel_depth 3"),
                                ("halo_depth", 4, "halo_depth 4")]:
        cfg = gol.native.EngineConfig()
        cfg.backend = "cpu"
        cfg.rule = BOSCO
        setattr(cfg, field, value)
        with pytest.raises(gol.native.GolError, match=names) as e:
            gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
        assert BOSCO in str(e.value)
    # (the HIP engine's refusal of the other kernels needs a device: test_gpu_ltl.py)


def test_more_ranks_are_refused(gol):
    ts = gol.parallel.thread_transports(2)
    with pytest.raises(ValueError, match="2 ranks") as e:
        gol.Simulation(64, ts[0], backend="cpu", rule=BOSCO)
    assert BOSCO in str(e.value)
    geo = gol.native.make_geometry(gol.native.make_decomposition(64, 2, False, "1d", "", 0), 0)
    cfg = gol.native.EngineConfig()
    cfg.backend = "cpu"
    cfg.rule = BOSCO
    with pytest.raises(gol.native.GolError, match="2 ranks") as e:
        gol.native.Engine.create(geo, cfg, ts[0])
    assert BOSCO in str(e.value)


def test_checkpoints_soups_and_evolve_are_refused(gol, tmp_path):
    import torch

    s = _sim(gol, 64, rule=BOSCO).init(5, seed=1)
    for name, call in {"checkpoint": lambda: s.checkpoint(str(tmp_path / "c")), "restore": lambda: s.restore(str(tmp_path / "c"))}.items():
        with pytest.raises(ValueError, match=name) as e:
            call()
        assert BOSCO in str(e.value) and "Larger than Life" in str(e.value)
    with pytest.raises(gol.native.GolError, match="save_checkpoint") as e:
        gol.native.save_checkpoint(s.engine, str(tmp_path / "c"), 0)
    assert BOSCO in str(e.value)
    with pytest.raises(gol.native.GolError, match="load_checkpoint") as e:
        gol.native.load_checkpoint(s.engine, str(tmp_path / "c"))
    assert BOSCO in str(e.value)
    assert not os.path.exists(str(tmp_path / "c.gol"))
    with pytest.raises(ValueError, match="Larger than Life") as e:
        gol.SoupBatch(4, 64, BOSCO, backend="cpu")
    assert BOSCO in str(e.value)
    with pytest.raises(ValueError, match="Larger than Life") as e:
        gol.ops.evolve(torch.zeros((64, 64), dtype=torch.uint8), 3, rule=BOSCO)
    assert BOSCO in str(e.value)


def test_cli_takes_the_rule_and_refuses_checkpoints(gol, gol_bin, tmp_path):
    """GOL_RULE through the CLI: a run under Bosco's rule writes the oracle's board as RLE; GOL_CHECKPOINT_EVERY and
    GOL_RESTART are refused by name."""
    env = dict(os.environ, GOL_BACKEND="cpu", GOL_RULE="bosco", GOL_RLE_OUT=str(tmp_path / "out.rle"))
    r = subprocess.run([gol_bin, "5", "64", "3", "256", "0"], env=env, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    back, rule = gol.ops.parse_rle((tmp_path / "out.rle").read_text())
    ref = _sim(gol, 64, rule=BOSCO).init(5).step(3).board()
    full = np.zeros_like(ref)
    full[: back.shape[0], : back.shape[1]] = back
    assert rule == BOSCO and np.array_equal(full, ref) and np.array_equal(ref, numpy_ltl(_sim(gol, 64).init(5).board(), BOSCO, 3))
    for extra in ({"GOL_CHECKPOINT_EVERY": "2", "GOL_CHECKPOINT": str(tmp_path / "ck")}, {"GOL_RESTART": str(tmp_path / "ck")}):
        r = subprocess.run([gol_bin, "5", "64", "3", "256", "0"], env=dict(env, **extra), capture_output=True, text=True, timeout=120,
                           cwd=str(tmp_path))
        assert r.returncode != 0 and "Larger than Life" in r.stderr and BOSCO in r.stderr, r.stdout + r.stderr
