"""Generations rules (B/S/C) without a GPU: the rule strings through the Python surface, the numpy oracle on
hand-made boards, and the CPU backend (cpu::superstep on planes) against the oracle: both boundaries, tail and
three-row boards, halo depths 1, 3 and 8, the state calls, stamping, RLE headers and every refusal.

Every comparison is exact; generations_cases.lively asks the oracle alone first."""
import numpy as np
import pytest

import generations_cases as gc
from gol_amd.ops import numpy_generations, numpy_step_rule, parse_generations_rule, parse_rule_states, random_board

ACCEPTED = [
    ("B2/S345/C4", "B2/S345/C4", 4), ("b2/s345/c4", "B2/S345/C4", 4), ("S345/B2/C4", "B2/S345/C4", 4),
    ("s543/b2/C4", "B2/S345/C4", 4), ("345/2/4", "B2/S345/C4", 4), ("/2/3", "B2/S/C3", 3), ("B2/S/C3", "B2/S/C3", 3),
    ("12/34/3", "B34/S12/C3", 3), ("B2/S345/C9", "B2/S345/C9", 9), ("B3/S23/C2", "B3/S23", 2), ("23/3/2", "B3/S23", 2),
    ("B36/S23", "B36/S23", 2), ("B2/S34H", "B2/S34H", 2), ("conway", "B3/S23", 2),
]
REJECTED = ["B2/S345/C0", "B2/S345/C1", "B2/S345/C10", "B2/S345/C99", "B2/S345/C04", "B2/S345/C", "B2/S345/C4V", "B2/S345/C4H",
            "B2/S34V/C4", "B0/S/C3", "/0/3", "345/2/", "345/2/1", "345/2/10", "345/2/04", "B2/S345/4", "B2/S345/C4 ", "B3/S23/",
            "B3/B3", "3/23", "B9/S/C3", "B22/S/C3"]


def _sim(gol, N, **kw):
    kw.setdefault("backend", "cpu")
    return gol.Simulation(N, **kw)


# ----- rule strings -----

@pytest.mark.parametrize("text,canonical,states", ACCEPTED)
def test_rule_accepted(gol, text, canonical, states):
    cfg = gol.native.EngineConfig()
    cfg.rule = text
    assert cfg.rule == canonical
    assert gol.native.parse_rule_states(text) == states == parse_rule_states(text)
    if "H" not in canonical:  # the Python parser agrees with the native one on the masks
        b, s, c = parse_generations_rule(text)
        cfg2 = gol.native.EngineConfig()
        cfg2.rule = canonical.split("/C")[0]
        assert (b, s) == gol.native.parse_rule(cfg2.rule) and c == states


@pytest.mark.parametrize("text", REJECTED)
def test_rule_rejected(gol, text):
    cfg = gol.native.EngineConfig()
    with pytest.raises(ValueError, match="invalid rule") as e:
        cfg.rule = text
    assert repr(text)[1:-1] in str(e.value)  # names the string
    with pytest.raises(ValueError):
        gol.native.parse_rule_states(text)
    with pytest.raises(ValueError):
        parse_generations_rule(text)


def test_existing_helpers_keep_their_results(gol):
    assert gol.native.parse_rule("B36/S23") == (0b1001000, 0b1100)
    assert gol.native.parse_rule_nbhd("B2/S34H") == (0b100, 0b11000, "H")
    assert gol.ops.parse_rule("S23/B36") == (0b1001000, 0b1100)
    assert gol.ops.rule_string("s23/b3") == "B3/S23"


# ----- the oracle -----

def test_oracle_by_hand():
    # Brian's Brain: two live cells side by side; the four cells with both as neighbours are born, the pair starts dying
    b = np.zeros((6, 6), np.uint8)
    b[2, 2] = b[2, 3] = 1
    g1 = numpy_generations(b, "B2/S/C3", 1)
    want = np.zeros((6, 6), np.uint8)
    want[2, 2] = want[2, 3] = 2
    want[1, 2] = want[1, 3] = want[3, 2] = want[3, 3] = 1
    assert np.array_equal(g1, want)
    g2 = numpy_generations(b, "B2/S/C3", 2)
    # the dying pair is dead and the four are dying; born are (0, 2), (0, 3), (4, 2), (4, 3), (2, 1) and (2, 4), each with two of them
    assert g2[2, 2] == 0 and g2[2, 3] == 0 and g2[1, 2] == 2 and (g2 == 1).sum() == 6 and g2[2, 1] == 1 and g2[0, 2] == 1
    # a dying cell counts as no neighbour, cannot be born, and decays whatever its neighbours do: C = 5 walks 2, 3, 4, 0
    c = np.zeros((5, 5), np.uint8)
    c[2, 2] = 2
    c[1, 1] = c[1, 3] = 1  # two live neighbours of (2, 2): a dead cell there would be born under B2
    seen = [int(numpy_generations(c, "B2/S345/C5", g)[2, 2]) for g in range(5)]
    assert seen[:4] == [2, 3, 4, 0]
    # the edge: a live pair on the top row of a bounded board has no births above it, on the torus it has
    d = np.zeros((5, 6), np.uint8)
    d[0, 2] = d[0, 3] = 1
    assert (numpy_generations(d, "B2/S/C3", 1, boundary="dead")[4] == 0).all()
    assert (numpy_generations(d, "B2/S/C3", 1, boundary="torus")[4] == 1).sum() == 2
    # two states: the life-like rule
    r = random_board(20, 33, 5)
    assert np.array_equal(numpy_generations(r, "B36/S23", 4), numpy_step_rule(r, "B36/S23", 4))
    with pytest.raises(ValueError, match="state 3"):
        numpy_generations(np.full((2, 2), 3, np.uint8), "B2/S/C3", 1)


# ----- the CPU engine -----

@pytest.mark.parametrize("hw", gc.BOARDS, ids=gc.board_id)
@pytest.mark.parametrize("R", gc.CPU_DEPTHS)
@pytest.mark.parametrize("rule", gc.CPU_RULES)
def test_cpu_engine(gol, rule, R, hw):
    for boundary in gc.BOUNDARIES:
        s = gc.run_case(lambda n, **kw: _sim(gol, n, **kw), rule, hw[0], hw[1], boundary, R, kernel="cpu")
        assert s.states == gc.STATES[rule]


def test_frogs_and_live_start(gol):
    """init(5) starts from live cells alone (the decay planes are zeroed); 40 generations of Frogs hold every state."""
    N, rule, gens = 100, gc.FROGS, 40
    start = gol.ops.initial_board(5, N, 1, True, 7)
    ref = numpy_generations(start, rule, gens)
    assert set(np.unique(ref).tolist()) == {0, 1, 2}
    s = _sim(gol, N, rule=rule, halo_depth=8).init(5, seed=7)
    gc.check(s, start)
    s.step(gens)
    gc.check(s, ref, "cpu")


@pytest.mark.parametrize("rule", gc.CPU_RULES)
def test_set_board_round_trip(gol, rule):
    H, W, C = 65, 137, gc.STATES[rule]
    states = np.random.default_rng(11).integers(0, C, size=(H, W), dtype=np.uint8)
    s = _sim(gol, H, width=W, rule=rule).init(5, seed=3)
    s.set_board(states)
    gc.check(s, states)
    assert np.array_equal(gol.ops.unpack_words(s.words(), W), (states == 1).astype(np.uint8))  # words(): the live plane
    bad = states.copy()
    bad[7, 9] = C
    with pytest.raises(ValueError, match=f"state {C}"):
        s.set_board(bad)
    gc.check(s, states)  # nothing was written
    with pytest.raises(ValueError, match=f"state {C}"):
        s.engine.set_state_tile(bad)
    gc.check(s, states)
    s.set_board(np.zeros((H, W), np.uint8))
    assert s.state_counts().tolist() == [H * W] + [0] * (C - 1)


@pytest.mark.parametrize("boundary", gc.BOUNDARIES)
def test_window_across_the_seams(gol, boundary):
    H, W, rule, gens = 65, 137, gc.C9, 5
    seed = gc.seed_of(H, W, rule, boundary)
    ref = gc.history(H, W, seed, rule, boundary, gens)[gens]
    s = gc.start_sim(_sim(gol, H, width=W, rule=rule, boundary=boundary, halo_depth=3), H, W, seed, rule)
    s.step(gens)
    assert np.array_equal(s.window(0, 0, H, W), ref)
    assert np.array_equal(s.window(10, 60, 20, 70), ref[10:30, 60:130])
    if boundary == "torus":
        got = s.window(-3, -5, 9, 12)  # across both seams: rows 62 .. 64, 0 .. 5, columns 132 .. 136, 0 .. 6
        want = np.roll(np.roll(ref, 3, axis=0), 5, axis=1)[:9, :12]
        assert np.array_equal(got, want) and set(np.unique(got).tolist()) >= {0, 1, 2}
    else:
        with pytest.raises(ValueError, match="does not lie inside"):
            s.window(-3, -5, 9, 12)


@pytest.mark.parametrize("mode", ["or", "replace", "xor", "clear"])
def test_stamp_keeps_the_invariant(gol, mode):
    """stamp() acts on the live plane; afterwards no cell is alive and dying: a stamped live cell has lost its counter,
    `replace` and `clear` leave the dying cells they do not make alive dying."""
    H, W, rule = 64, 100, gc.STARWARS
    seed = gc.seed_of(H, W, rule, "torus")
    before = gc.start_states(H, W, seed, 4)
    pat = random_board(9, 70, 21)
    s = gc.start_sim(_sim(gol, H, width=W, rule=rule), H, W, seed, rule)
    s.stamp(pat, at=(60, 60), mode=mode)  # across both seams
    live = (before == 1).astype(np.uint8)
    rr, cc = np.ix_(np.arange(60, 69) % H, np.arange(60, 130) % W)
    sub = live[rr, cc]
    live[rr, cc] = {"or": sub | pat, "replace": pat, "xor": sub ^ pat, "clear": sub & (1 - pat)}[mode]
    want = np.where(live == 1, 1, np.where(before >= 2, before, 0)).astype(np.uint8)
    if mode != "clear":  # some stamped cell was dying: its counter had to be cleared
        assert ((want == 1) & (before >= 2)).any()
    gc.check(s, want)
    ref = numpy_generations(want, rule, 7)
    s.step(7)
    gc.check(s, ref)


def test_from_rle_with_a_generations_header(gol, tmp_path):
    text = "x = 3, y = 2, rule = 345/2/4\nboo$2ob!\n"
    path = tmp_path / "sw.rle"
    path.write_text(text)
    s = gol.Simulation.from_rle(str(path), 40, backend="cpu")
    assert s.states == 4 and s.config.rule == "B2/S345/C4"
    start = np.zeros((40, 40), np.uint8)
    start[19, 18:21] = [0, 1, 1]
    start[20, 18:21] = [1, 1, 0]
    gc.check(s, start)
    s.step(9)
    gc.check(s, numpy_generations(start, "B2/S345/C4", 9))
    with pytest.raises(ValueError, match="names rule B2/S345/C4"):
        gol.Simulation.from_rle(str(path), 40, backend="cpu", rule="B2/S345/C5")
    # multi-state cell tokens stay refused
    with pytest.raises(ValueError):
        gol.native.parse_rle("x = 2, y = 1, rule = B2/S345/C4\nAB!\n")
    with pytest.raises(ValueError):
        gol.native.parse_rle("x = 2, y = 1, rule = B2/S345/C4\n.A!\n")


# ----- refusals -----

REFUSED = [
    ({"census": True}, "census"), ({"signature": True}, "signature"), ({"film": (0, 0, 8, 8)}, "film"),
    ({"density_film": (8, 64)}, "density_film"), ({"envelope": True}, "envelope"), ({"compat": True}, "compat"),
    ({"subtiles": 2}, "subtiles"), ({"self_exchange": True}, "self_exchange"), ({"force_split": True}, "force_split"),
    ({"backend": "hip", "kernel": "temporal"}, "temporal"), ({"backend": "hip", "kernel": "tile"}, "tile"),
    ({"backend": "hip", "kernel": "lds"}, "lds"),
]


@pytest.mark.parametrize("kw,names", REFUSED, ids=[n for _, n in REFUSED])
def test_constructor_refusals(gol, kw, names):
    kw = dict(kw)
    kw.setdefault("backend", "cpu")
    with pytest.raises(ValueError, match=names) as e:
        gol.Simulation(64, rule="B2/S345/C4", **kw)
    assert "B2/S345/C4" in str(e.value)


def test_kernel_depth_refusal(gol):
    assert [gol.native.max_generations_depth(c) for c in range(3, 10)] == [8, 5, 5, 2, 2, 2, 2]
    for c in (2, 10):
        with pytest.raises(ValueError):
            gol.native.max_generations_depth(c)
    with pytest.raises(ValueError, match="kernel_depth 6") as e:
        gol.Simulation(64, rule="B2/S345/C4", backend="hip", kernel_depth=6)
    assert "B2/S345/C4" in str(e.value) and "5 generations" in str(e.value)


def test_engine_refusals(gol):
    """The engine's own constructor refuses what the Python one does, each error naming the option and the rule."""
    geo = gol.native.make_geometry(gol.native.make_decomposition(64, 1, False, "1d", "", 0), 0)
    for field, value, names in [("census", True, "census"), ("signature", True, "signature"), ("film", (0, 0, 8, 8), "film"),
                                ("density_film", (8, 64), "density_film"), ("envelope", True, "envelope"),
                                ("compat", True, "compat"), ("subtiles", 2, "subtiles"), ("self_exchange", True, "self_exchange"),
                                ("force_split", True, "force_split")]:
        cfg = gol.native.EngineConfig()
        cfg.backend = "cpu"
        cfg.rule = "B2/S/C3"
        setattr(cfg, field, value)
        with pytest.raises(gol.native.GolError, match=names) as e:
            gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
        assert "B2/S/C3" in str(e.value)


def test_more_ranks_are_refused(gol):
    ts = gol.parallel.thread_transports(2)
    with pytest.raises(ValueError, match="2 ranks"):
        gol.Simulation(64, ts[0], backend="cpu", rule="B2/S/C3")
    geo = gol.native.make_geometry(gol.native.make_decomposition(64, 2, False, "1d", "", 0), 0)
    cfg = gol.native.EngineConfig()
    cfg.backend = "cpu"
    cfg.rule = "B2/S/C3"
    with pytest.raises(gol.native.GolError, match="2 ranks"):
        gol.native.Engine.create(geo, cfg, ts[0])


def test_calls_refused_in_this_version(gol, tmp_path):
    import torch

    s = _sim(gol, 64, rule="B2/S345/C4").init(5, seed=1)
    t = torch.zeros((64, 64), dtype=torch.uint8)
    calls = {
        "checkpoint": lambda: s.checkpoint(str(tmp_path / "c")),
        "restore": lambda: s.restore(str(tmp_path / "c")),
        "save_rle": lambda: s.save_rle(str(tmp_path / "b.rle")),
        "dump": lambda: s.dump(str(tmp_path / "d.txt")),
        "board_tensor": lambda: s.board_tensor(),
        "load_tensor": lambda: s.load_tensor(t),
        "window_tensor": lambda: s.window_tensor(0, 0, 8, 8),
        "match_tensor": lambda: s.match_tensor(np.ones((2, 2), np.uint8)),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=name) as e:
            call()
        assert "B2/S345/C4" in str(e.value) and "Generations" in str(e.value)
    # the native calls behind them refuse as well
    for call in (lambda: s.engine.read_tile_cells(t.data_ptr(), 0, t.numel()), lambda: s.engine.write_tile_cells(t.data_ptr(), 0, t.numel()),
                 lambda: s.engine.read_window_cells(0, 0, 8, 8, t.data_ptr(), 0, 64)):
        with pytest.raises(ValueError, match="Generations"):
            call()
    with pytest.raises(gol.native.GolError, match="Generations"):
        gol.native.save_checkpoint(s.engine, str(tmp_path / "c"), 0)
    with pytest.raises(ValueError, match="Generations"):
        gol.SoupBatch(4, 64, "B2/S345/C4", backend="cpu")
    with pytest.raises(ValueError, match="Generations"):
        gol.ops.evolve(torch.zeros((64, 64), dtype=torch.uint8), 3, rule="B2/S/C3")
    # a two-state simulation has no state calls
    p = _sim(gol, 64).init(5, seed=1)
    assert p.states == 2 and p.stats()["states"] == 2
    with pytest.raises(ValueError, match="state_counts"):
        p.state_counts()
    with pytest.raises(ValueError, match="two states"):
        p.engine.state_tile()


def test_live_plane_readers(gol):
    """population, density, fingerprint, signature, match and snapshot_diff read the live cells (state 1)."""
    H, W, rule = 64, 128, gc.C5
    seed = gc.seed_of(H, W, rule, "torus")
    states = gc.start_states(H, W, seed, 5)
    live = (states == 1).astype(np.uint8)
    s = gc.start_sim(_sim(gol, H, width=W, rule=rule), H, W, seed, rule)
    p = _sim(gol, H, width=W)  # a two-state board holding the live cells
    p.init(0)
    p.set_board(live)
    assert s.population() == p.population() == int(live.sum())
    assert s.fingerprint() == p.fingerprint() and s.signature() == p.signature()
    assert np.array_equal(s.density(16, 64), p.density(16, 64))
    assert s.count_matches(np.ones((1, 1), np.uint8), margin=0) == int(live.sum())
    s.snapshot()
    assert s.snapshot_diff() == 0
