"""Envelope mode on the HIP backend: the kernel step_envelope<K> (envelope_kernel.hip, nbhd_envelope_kernel.hip) under
every schedule the census kernel runs under -- pass depths, board sizes, wrap and ghost rows, both boundaries, wide
boards with full-width segments, multi-pass supersteps, thread ranks sharing the GPU, rank grids, the 1-rank RCCL
communicator, the other neighbourhoods -- against the numpy oracle ``numpy_envelope``.

Every comparison is exact, and each also asserts the ``envelope@`` kernel, ``stats()["envelope"]`` and that the final
board is the oracle's (envelope_cases.check).  The oracle-only conditions of envelope_cases.lively come first: with
passes of two generations or more, an envelope that misses the generations between the pass ends is wrong."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import envelope_cases as ec
import film_cases as fc
import wide_cases as wc
from gol_amd.ops import initial_board, numpy_envelope
from gol_amd.ops.rle import pattern_cells

pytestmark = pytest.mark.gpu


def _sim(gol, N, **kw):
    kw.setdefault("backend", "hip")
    kw.setdefault("device", 0)
    return gol.Simulation(N, **kw)


def test_depths_are_instantiated(gol):
    assert gol.native.max_envelope_depth() == 8


@pytest.mark.parametrize("N", ec.SIZES)
@pytest.mark.parametrize("K", ec.DEPTHS)
def test_sweep(gol, K, N):
    """Every pass depth on every size class (wrap rows on boards shorter than the pass; tail words of 1, 63 and 9 cells;
    packed segments in the per-lane runner; several blocks): 2K + 1 generations, a full pass, a second, a remainder."""
    ec.run_sweep_case(lambda n, **kw: _sim(gol, n, **kw), K, N, kernel=f"envelope@{K}" if N >= 63 else "envelope@")  # (a 1-, 2- or 3-row board clamps the depth)


WIDE = [wc.S3968, wc.S3950, wc.S4096, wc.S3969, wc.S8000, wc.S7936]


@pytest.mark.parametrize("shape", WIDE, ids=[wc.shape_id(s) for s in WIDE])
@pytest.mark.parametrize("K", ec.DEPTHS)
def test_wide(gol, K, shape):
    """Full-width segments in the scalar runner (wide_cases.py tells what each shape gives)."""
    gens, rule = 2 * K + 1, ec.HIGHLIFE
    H, W = shape.H, shape.W
    for boundary in ec.BOUNDARIES:
        h = ec.history(H, W, wc.SEED, rule, boundary, ec.SWEEP_GENS)
        assert ec.lively(H, W, wc.SEED, rule, boundary, gens, K, ec.SWEEP_GENS)
        s = _sim(gol, H, width=W, rule=rule, boundary=boundary, halo_depth=K, kernel_depth=K, envelope=True).init(5, seed=wc.SEED)
        s.step(gens)
        ec.check(s, 0, h.envelope(gens), h.board(gens), f"envelope@{K}")


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("R", [16, 24])
def test_multipass_supersteps(gol, R, graph):
    """Supersteps of two and three passes of depth 8: the extension rows the earlier passes compute beyond the tile are
    not owned; launches are eager whatever GOL_GRAPH says."""
    for s in ec.run_multipass_case(lambda n, **kw: _sim(gol, n, **kw), R, kernel="envelope@8", graph=bool(graph)):
        st = s.stats()
        assert st["depth"] == R and st["kernel_depth"] == 8 and st["graph_launches"] == 0, st


@pytest.mark.parametrize("N", [64, 65, 137])
@pytest.mark.parametrize("K", ec.DEPTHS)
@pytest.mark.parametrize("rule", ec.NBHD_RULES)
def test_neighbourhoods(gol, rule, K, N):
    ec.run_nbhd_case(lambda n, **kw: _sim(gol, n, **kw), rule, K, N, kernel=f"envelope@{K}")


@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
def test_life_cycle(gol, tmp_path, boundary):
    ec.run_life_cycle(lambda n, **kw: _sim(gol, n, **kw), tmp_path, boundary, kernel="envelope@8")


def test_run_hint_prediction_leaves_nothing(gol):
    N, gens, rule = 200, 21, ec.HIGHLIFE
    h = ec.history(N, N, 3, rule, "torus", gens)
    s = _sim(gol, N, rule=rule, halo_depth=8, run_hint=gens, envelope=True).init(5, seed=3)
    assert s.generation == 0
    ec.check(s, 0, h.board(0), h.board(0), "envelope@8")
    s.step(gens)
    assert ec.lively(N, N, 3, rule, "torus", gens, 8)
    ec.check(s, 0, h.envelope(gens), h.board(gens))


@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
def test_views(gol, boundary):
    ec.run_views(lambda n, **kw: _sim(gol, n, **kw), boundary, fc.WINDOWS, fc.WRAPPING)


@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
@pytest.mark.parametrize("name,kw", [("1d3", {}), ("1d4", {"schedule": "split"}), ("1d4", {"schedule": "full"}), ("2x2", {}),
                                     ("3x3", {})], ids=["1d3", "P4-split", "P4-full", "2x2", "3x3"])
def test_thread_ranks(gol, name, kw, boundary):
    """Thread ranks on hip and on cpu against numpy: strips under the split and the full schedule, 2-D grids; 23
    generations in two step() calls, supersteps of two passes and remainders.  The assembled envelope() tiles, an
    envelope_window over the point where tiles meet and the global count, on every rank."""
    P, grid, H, W, windows = fc.RANK_CASES[name]
    rule, rect = ec.HIGHLIFE, windows[0]
    h = ec.history(H, W, ec.RANK_SEED, rule, boundary, ec.RANK_GENS)
    assert ec.lively(H, W, ec.RANK_SEED, rule, boundary, ec.RANK_GENS, 8)
    for backend in ("hip", "cpu"):
        parts = wc.run_ranks(gol, P, H, W, backend, script=ec.rank_script(rect), rule=rule, boundary=boundary, envelope=True,
                             **grid, **kw)
        ec.check_rank_parts(H, W, parts, h, rect)
        if backend == "hip":
            for p in parts:
                st = p.result[4]
                assert st["kernel"].startswith("envelope@"), st
                if "schedule" in kw:
                    assert ("+boundary:envelope@" in st["kernel"]) == (kw["schedule"] == "split"), st


@pytest.fixture(scope="module")
def rccl(gol):
    """One 1-rank RCCL communicator shared by the module (communicator init costs seconds)."""
    gol.native.hip_set_device(0)
    t = gol.native.make_rccl_transport(gol.native.SelfTransport())
    assert t.size() == 1 and t.device_buffers() and t.name().startswith("rccl")
    yield t


@pytest.mark.parametrize("kw", [{}, {"decomp": "2d"}], ids=["1d", "2d"])
def test_rccl_self(gol, rccl, kw):
    N, R, gens, rule, boundary = 256, 16, 40, ec.HIGHLIFE, "torus"
    s = gol.Simulation(N, rccl, backend="hip", device=0, self_exchange=True, rule=rule, boundary=boundary, halo_depth=R,
                       kernel_depth=8, subtiles=0, envelope=True, **kw)
    s.init(5, seed=R)
    s.step(gens)
    st = s.stats()
    assert st["exchanges"] >= 3 and st["halo_bytes"] > 0, st
    h = ec.history(N, N, R, rule, boundary, gens)
    assert ec.lively(N, N, R, rule, boundary, gens, 8)
    ec.check(s, 0, h.envelope(gens), h.board(gens), "envelope@8")
    s.synchronize()


def test_refusals(gol):
    for kw, word in [({"census": True}, "census"), ({"signature": True}, "signature"), ({"film": (0, 0, 8, 8)}, "film"),
                     ({"density_film": (8, 64)}, "density_film"), ({"compat": True}, "compat"), ({"subtiles": 2}, "subtiles=2"),
                     ({"kernel_depth": 9}, "kernel_depth 9")] + [
                         ({"kernel": k}, k) for k in ("temporal", "tile", "pipe", "resident", "lds")]:
        with pytest.raises(ValueError) as e:
            _sim(gol, 64, envelope=True, **kw)
        assert word in str(e.value) and "envelope" in str(e.value), str(e.value)
    plain = _sim(gol, 64).init(5)
    assert plain.stats()["envelope"] is None
    for call in (plain.envelope, lambda: plain.envelope_window(0, 0, 4, 4), lambda: plain.envelope_density(8, 64),
                 plain.envelope_population, plain.envelope_clear):
        with pytest.raises(ValueError) as e:
            call()
        assert "envelope mode" in str(e.value)
    with pytest.raises(gol.native.GolError) as e:
        plain.engine.envelope()
    assert "envelope mode" in str(e.value)
    # the engine on its own refuses the same
    dec = gol.native.make_decomposition(64, 1, False, "1d", "", 0)
    geo = gol.native.make_geometry(dec, 0)
    for attr, value, word in [("kernel_depth", 9, "kernel_depth 9"), ("kernel", "temporal", "temporal"), ("kernel", "lds", "lds"),
                              ("census", True, "census"), ("signature", True, "signature"), ("film", (0, 0, 8, 8), "film"),
                              ("density_film", (8, 64), "density_film"), ("compat", True, "GOL_COMPAT"),
                              ("subtiles", 2, "GOL_SUBTILES=2")]:
        cfg = gol.native.EngineConfig()
        cfg.backend, cfg.device = "hip", 0
        cfg.envelope = True
        setattr(cfg, attr, value)
        with pytest.raises(gol.native.GolError) as e:
            gol.native.Engine.create(geo, cfg, gol.native.SelfTransport())
        assert word in str(e.value) and "envelope" in str(e.value), str(e.value)


def test_ranks_disagree(gol):
    """Every rank raises at init and none hangs."""
    P = 3
    ts = gol.parallel.p2p_thread_transports(P)
    errs = [None] * P

    def rank_main(r):
        try:
            gol.Simulation(32, ts[r], backend="hip", device=0, envelope=r != 1).init(5)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert all(e is not None and "envelope" in str(e) and "disagree" in str(e) for e in errs), errs


# ----- the CLI -----

def _cli(gol_bin, args, cwd, **env):
    e = dict(os.environ)
    e["GOL_BACKEND"] = "hip"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "GOL_RULE", "GOL_NRANKS", "GOL_BOUNDARY",
              "GOL_PATTERN_FILE", "GOL_PATTERN_AT", "GOL_RLE_OUT", "GOL_CENSUS", "GOL_CENSUS_OUT", "GOL_COMPAT", "GOL_SUBTILES",
              "GOL_SIGNATURE", "GOL_SIGNATURE_OUT", "GOL_FILM", "GOL_FILM_OUT", "GOL_DENSITY_FILM", "GOL_DENSITY_FILM_OUT",
              "GOL_ENVELOPE", "GOL_ENVELOPE_OUT", "GOL_SOUPS"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([gol_bin, *map(str, args)], cwd=cwd, env=e, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("boundary", ec.BOUNDARIES)
def test_cli_envelope_out(gol, gol_bin, tmp_path, boundary):
    N, gens, rule = 137, 21, "B36/S23"
    r = _cli(gol_bin, [5, N, gens, 64, 0], tmp_path, GOL_ENVELOPE_OUT=tmp_path / "env.rle", GOL_RULE=rule, GOL_BOUNDARY=boundary,
             GOL_METRICS_JSON=tmp_path / "m.json")
    assert r.returncode == 0, r.stderr
    ref, last = numpy_envelope(initial_board(5, N, 1, True), rule, gens, bounded=boundary == "dead", return_board=True)
    assert not np.array_equal(ref, last) and not ref.all()
    p = gol.native.parse_rle((tmp_path / "env.rle").read_text())
    assert p.rule == rule and (p.rows, p.cols) == (N, N) and p.topology == ("P" if boundary == "dead" else "")
    assert np.array_equal(pattern_cells(p), ref)
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["envelope"] == 0 and m["kernel"].startswith("envelope@"), m


def test_cli_unwritable_path(gol_bin, tmp_path):
    bad = tmp_path / "no" / "such" / "dir" / "env.rle"
    r = _cli(gol_bin, [5, 64, 5, 64, 0], tmp_path, GOL_ENVELOPE_OUT=bad)
    assert r.returncode != 0 and str(bad) in r.stderr and "GOL_ENVELOPE_OUT" in r.stderr
