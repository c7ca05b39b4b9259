"""Von Neumann (``V``) and hexagonal (``H``) rules on the HIP backend: the generic-rule kernels with the gates of
nbhd_gates.hpp (step_rule, step_rule_bounded, step_census, step_signature on the two neighbourhoods) under every engine
path they take, bit for bit against the numpy oracles, which count neighbours by shifted adds over the literal 3 x 3
masks.  Every reference is computed once and left read-only; where the board is not tiny, the Moore oracle for the same
B/S lists must give another board, so a kernel that ignored the suffix could not pass."""
import functools

import numpy as np
import pytest

import grid_cases as gc
import wide_cases as wc
from gol_amd.ops import (
    numpy_signature,
    numpy_step_rule,
    numpy_step_rule_bounded,
    random_board,
    rule_string,
)

pytestmark = pytest.mark.gpu

HEX, VON = "B2/S34H", "B13/S13V"
RULES = [HEX, VON, "B1/SH", "B1/SV"]
BOUNDARIES = ["torus", "dead"]
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8]
# the neighbourhoods as literals (rows downward, columns rightward)
MASKS = {"V": np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], np.uint8), "H": np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1]], np.uint8)}


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


def _step(boundary):
    return numpy_step_rule_bounded if boundary == "dead" else numpy_step_rule


def moore_of(rule):
    return rule_string(rule)[:-1]


@functools.lru_cache(maxsize=None)
def series(H, W, seed, rule, boundary, gens):
    """``(boards, pops, sigs)`` of generations 1 .. gens of the H x W random board of ``seed``: the boards after every odd
    generation and the last, the populations and the signatures, one numpy generation at a time.  On a board that is
    not tiny, the Moore rule of the same lists differs after one generation."""
    b = random_board(H, W, seed)
    if min(H, W) > 3:
        assert not np.array_equal(_step(boundary)(b, rule, 1), _step(boundary)(b, moore_of(rule), 1))
    boards, pops, sigs = {}, [], []
    for g in range(1, gens + 1):
        b = _step(boundary)(b, rule, 1)
        pops.append(int(b.sum()))
        sigs.append(numpy_signature(b))
        if g % 2 or g == gens:
            b.setflags(write=False)
            boards[g] = b
    return boards, np.array(pops, np.uint64), np.array(sigs, np.uint64)


def run_and_check(gol, H, W, seed, rule, boundary, gens, total, **kw):
    s = _sim(gol, H, width=W, rule=rule, boundary=boundary, **kw).init(5, seed=seed)
    st = s.stats()
    assert st["kernel"].startswith("rule@") and st["rule"] == rule and st["boundary"] == boundary, st
    s.step(gens)
    assert np.array_equal(s.board(), series(H, W, seed, rule, boundary, total)[0][gens]), (rule, boundary, H, W, kw)
    return s, st


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000])
@pytest.mark.parametrize("K", DEPTHS)
def test_sweep(gol, K, N):
    """step_rule and step_rule_bounded at every instantiated depth on every size class, 2K + 1 generations."""
    gens, total = 2 * K + 1, 2 * max(DEPTHS) + 1
    for boundary in BOUNDARIES:
        for rule in RULES:
            _, st = run_and_check(gol, N, N, N, rule, boundary, gens, total, halo_depth=K, kernel_depth=K)
            assert N < 63 or st["kernel_depth"] == K, st


def _single_bit_rules():
    out = []
    for sfx, top in (("V", 4), ("H", 6)):
        out += [f"B{c}/S{sfx}" for c in range(1, top + 1)] + [f"B/S{c}{sfx}" for c in range(top + 1)]
    return out


@functools.lru_cache(maxsize=None)
def lively(rule, N, seed, gens):
    """``rule``, or ``rule`` with B1 added where the board of the rule itself is dead after ``gens`` generations."""
    b = numpy_step_rule(random_board(N, N, seed), rule, gens)
    if b.any():
        return rule
    birth, rest = rule_string(rule)[1:].split("/")
    return rule_string(f"B1{birth.replace('1', '')}/{rest}")


@pytest.mark.parametrize("K", [8, 3])
@pytest.mark.parametrize("rule", _single_bit_rules())
def test_single_bit_rules(gol, rule, K):
    """Every entry of each neighbourhood's rule table on its own: every leaf of the mux tree is selected alone."""
    N, gens = 137, 2 * K + 1
    rule = lively(rule, N, 1, gens)
    for boundary in BOUNDARIES:
        run_and_check(gol, N, N, 1, rule, boundary, gens, gens, halo_depth=K, kernel_depth=K)


def _placed(mask, H, W, r, c, bounded):
    want = np.zeros((H, W), np.uint8)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if mask[dy + 1, dx + 1]:
                y, x = r + dy, c + dx
                if bounded and not (0 <= y < H and 0 <= x < W):
                    continue
                want[y % H, x % W] = 1
    return want


@pytest.mark.parametrize("c", [0, 1, 62, 63, 64, 65, 128, 129])
def test_seams(gol, c):
    """One live cell in row 0 of a 130-column, 7-row board under B1/S: even and odd halves, the lane seam, the x-wrap
    through the masked tail word and the y-wrap.  Generation 1 is the literal mask around the cell (both masks are
    point-symmetric), on a bounded board without the cells beyond the edge."""
    H, W = 7, 130
    start = np.zeros((H, W), np.uint8)
    start[0, c] = 1
    for sfx in ("H", "V"):
        rule = f"B1/S{sfx}"
        for boundary in BOUNDARIES:
            literal = _placed(MASKS[sfx], H, W, 0, c, boundary == "dead")
            assert np.array_equal(_step(boundary)(start, rule, 1), literal)
            for K, gens in ((1, 1), (3, 3)):
                s = _sim(gol, H, width=W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K).init(0)
                s.set_board(start)
                s.step(gens)
                got = s.board()
                assert np.array_equal(got, _step(boundary)(start, rule, gens)), (rule, boundary, K, c)
                if gens == 1:
                    assert np.array_equal(got, literal)
                if boundary == "torus":  # (in a corner of a bounded board the masks' difference can lie beyond the edge)
                    assert not np.array_equal(got, numpy_step_rule(start, "B1/S", gens))


@pytest.mark.parametrize("shape", [wc.S3969, wc.S3968], ids=wc.shape_id)
def test_wide(gol, shape):
    """Full-width segments: halo lanes 0 and 63 (3968 columns), a tail word of one cell (3969)."""
    K = 8
    for boundary in BOUNDARIES:
        for rule in (HEX, VON):
            run_and_check(gol, shape.H, shape.W, wc.SEED, rule, boundary, 2 * K + 1, 2 * K + 1, halo_depth=K, kernel_depth=K)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("R", [16, 24])
def test_multipass_supersteps(gol, R, graph):
    N, gens = 200, 10 * R + 5  # (a graph is replayed from the third superstep of a kind on)
    for rule, boundary in ((HEX, "torus"), (VON, "torus"), (HEX, "dead")):
        s, st = run_and_check(gol, N, N, 6, rule, boundary, gens, gens, halo_depth=R, kernel_depth=8, graph=graph)
        assert st["depth"] == R and st["kernel_depth"] == 8, st
        after = s.stats()
        assert (after["graph_launches"] >= 1) if graph else (after["graph_launches"] == 0), after


@pytest.mark.parametrize("N", [65, 137])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_census(gol, K, N):
    gens = 2 * K + 1
    for boundary in BOUNDARIES:
        for rule in (HEX, VON):
            boards, pops, _ = series(N, N, N, rule, boundary, gens)
            s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, census=True).init(5, seed=N)
            assert s.stats()["kernel"].startswith("census@") and s.stats()["rule"] == rule, s.stats()
            s.step(gens)
            start, got = s.census()
            assert start == 0 and np.array_equal(got, pops), (got.tolist(), pops.tolist())
            assert int(got[-1]) == s.population() and len(set(got.tolist())) >= 2
            assert np.array_equal(s.board(), boards[gens])


@pytest.mark.parametrize("N", [65, 137])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_signatures(gol, K, N):
    gens = 2 * K + 1
    for boundary in BOUNDARIES:
        for rule in (HEX, VON):
            boards, pops, sigs = series(N, N, N, rule, boundary, gens)
            s = _sim(gol, N, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, signature=True).init(5, seed=N)
            assert s.stats()["kernel"].startswith("sig@") and s.stats()["rule"] == rule, s.stats()
            s.step(gens)
            start, got, got_pops = s.signatures()
            assert start == 0 and np.array_equal(got_pops, pops), (got_pops.tolist(), pops.tolist())
            assert np.array_equal(got, sigs), ([hex(v) for v in got.tolist()], [hex(v) for v in sigs.tolist()])
            assert int(got[-1]) == s.signature() and int(got_pops[-1]) == s.population() and len(set(got.tolist())) >= 2
            assert np.array_equal(s.board(), boards[gens])


CYCLE_PATTERN = np.array([[1, 1, 0, 0], [1, 1, 1, 1], [0, 1, 1, 0], [1, 0, 0, 0]], np.uint8)


def test_find_cycle(gol):
    """A small pattern on a 64 x 64 torus under B2/S34H against a brute-force numpy loop."""
    rule, N = "B2/S34H", 64
    board = np.zeros((N, N), np.uint8)
    board[30:34, 30:34] = CYCLE_PATTERN
    seen, b, want = {board.tobytes(): 0}, board, None
    for g in range(1, 2001):
        b = numpy_step_rule(b, rule, 1)
        if b.tobytes() in seen:
            want = (seen[b.tobytes()], g - seen[b.tobytes()])
            break
        seen[b.tobytes()] = g
    assert want is not None
    s = _sim(gol, N, rule=rule, halo_depth=8, signature=True).init(0)
    s.set_board(board)
    got = s.find_cycle(2000, chunk=50)
    assert got is not None and (got.transient, got.period) == want, (got, want)
    assert got.population == int(numpy_step_rule(board, rule, got.generation).sum())


@pytest.mark.parametrize("kw", [{"schedule": "split"}, {"schedule": "full"}, {"decomp": "2d", "grid": "2x2"}],
                         ids=["1d-split", "1d-full", "2x2"])
@pytest.mark.parametrize("H,W", [(96, 4096), (200, 200)])
def test_thread_ranks(gol, H, W, kw):
    """P = 4 against numpy and the CPU backend."""
    for rule, boundary in ((HEX, "torus"), (VON, "dead")):
        ref = series(H, W, wc.SEED, rule, boundary, wc.RANK_GENS)[0][wc.RANK_GENS]
        parts = wc.run_ranks(gol, 4, H, W, "hip", rule=rule, boundary=boundary, **kw)
        assert all(p.stats["kernel"].startswith("rule@") and p.stats["rule"] == rule for p in parts)
        assert np.array_equal(wc.assemble(H, W, parts), ref), (rule, boundary)
        cpu = wc.run_ranks(gol, 4, H, W, "cpu", rule=rule, boundary=boundary, **kw)
        assert np.array_equal(wc.assemble(H, W, cpu), ref), (rule, boundary)


def test_grid_3x3(gol):
    case = gc.CASES[0]
    for rule, boundary in ((HEX, "dead"), (VON, "torus")):
        ref = series(case.H, case.W, gc.SEED, rule, boundary, gc.GENS)[0][gc.GENS]
        gc.check_board(case, gc.run_ranks(gol, case, "hip", rule=rule, boundary=boundary), ref)
        gc.check_board(case, gc.run_ranks(gol, case, "cpu", rule=rule, boundary=boundary), ref)


@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


@pytest.mark.parametrize("kw", [{"schedule": "full"}, {"decomp": "2d"}], ids=["1d", "2d"])
def test_rccl_self(gol, rccl, kw):
    N, R = 512, 8
    gens = 3 * R + 5
    s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=HEX, halo_depth=R, subtiles=0, **kw)
    s.init(5, seed=R)
    s.step(gens)
    st = s.stats()
    got = s.board()
    s.synchronize()
    assert st["kernel"].startswith("rule@") and st["rule"] == HEX and st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
    assert np.array_equal(got, series(N, N, R, HEX, "torus", gens)[0][gens])


def test_stats_and_refusals(gol):
    for rule in (HEX, VON):
        s = _sim(gol, 128, rule=rule.lower()).init(5, seed=2)
        st = s.stats()
        assert st["rule"] == rule and st["rule"][-1] in "HV" and st["kernel"].startswith("rule@"), st
        for kw, word in [({"compat": True}, "B3/S23"), ({"subtiles": 2}, "B3/S23"), ({"kernel": "temporal"}, "B3/S23 only"),
                         ({"kernel": "tile"}, "B3/S23 only")]:
            with pytest.raises(ValueError) as e:
                _sim(gol, 128, rule=rule, **kw)
            assert word in str(e.value) and rule in str(e.value)
        for field, value in [("compat", True), ("subtiles", 2), ("kernel", "resident")]:
            cfg = gol.native.EngineConfig()
            cfg.backend, cfg.rule, cfg.device = "hip", rule, 0
            setattr(cfg, field, value)
            with pytest.raises(gol.native.GolError) as e:
                gol.native.Engine.create(s.geometry, cfg, s.transport)
            assert rule in str(e.value)
    with pytest.raises(ValueError) as e:
        _sim(gol, 128, rule="B5/S2V")
    assert "B5/S2V" in str(e.value)
