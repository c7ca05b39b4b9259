"""Times the tensor readers and writers against the host paths they replace (docs/PERFORMANCE.md, "Device tensors"), on
one GPU, rule B36/S23 after init(5).  Within a section the variants run interleaved (old, new, yardstick, old, ...), each
call bracketed by device synchronisation; median, min and max of --reps timed rounds after --warmup rounds.

  board     board() [host: D2H of the packed tile, unpacked by numpy] against board_tensor(uint8) and (float32) into a
            preallocated tensor, beside the yardstick: a device-to-device copy (torch copy_, hipMemcpyDtoD) of the
            result's byte count; "share" is yardstick time / board_tensor time
  load      set_board(numpy array) against load_tensor(uint8 CUDA tensor)
  film      step(n); film() against step_film(n) for a 512 x 512 window at 8192^2 (n = 1000), and per generation for a
            2048 x 2048 window (n = --film-gens); step(n) alone is the floor both share
  soups     SoupBatch.boards() against boards_tensor() for 16384 soups of 64 x 64
  evolve    ops.evolve on a (16384, 64, 64) uint8 CUDA tensor for 1000 generations against the batched conv2d loop of
            ops.torch_step_rule on the same tensor (--conv-gens generations, scaled), results compared

The old paths are untouched by the tensor layer, so their times here are the parent's on the same box.

    python tools/measure_tensors.py [--sizes 8192,32768] [--reps 5] [--sections board,load,film,soups,evolve]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="8192,32768")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--film-gens", type=int, default=200)
ap.add_argument("--conv-gens", type=int, default=50)
ap.add_argument("--soups", type=int, default=16384)
ap.add_argument("--sections", default="board,load,film,soups,evolve")
ap.add_argument("--rule", default="B36/S23")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gol_amd  # noqa: E402

DEV = "cuda:0"


def sync():
    torch.cuda.synchronize()


def interleaved(variants, reps=None, before=None):
    """{name: fn} timed round-robin; ``before[name]`` runs untimed in front of the variant."""
    ts = {k: [] for k in variants}
    reps = reps or a.reps
    for i in range(a.warmup + reps):
        for name, fn in variants.items():
            if before and name in before:
                before[name]()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= a.warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ts.items()}


def emit(section, **kw):
    print(json.dumps(dict(section=section, **kw)), flush=True)


def board_sections(N, sections):
    sim = gol_amd.Simulation(N, backend="hip", device=0, rule=a.rule).init(5, seed=1)
    sim.step(3)
    if "board" in sections:
        for dtype in (torch.uint8, torch.float32):
            out = torch.empty((N, N), dtype=dtype, device=DEV)
            src = torch.ones((N, N), dtype=dtype, device=DEV)
            dst = torch.empty_like(src)
            v = {"board_tensor": lambda: sim.board_tensor(out=out), "d2d_copy": lambda: dst.copy_(src)}
            if dtype == torch.uint8:
                v = {"board": sim.board, **v}
            r = interleaved(v)
            nbytes = out.numel() * out.element_size()
            r["bytes"] = nbytes
            r["board_tensor_GBps"] = round(nbytes / r["board_tensor"]["median_ms"] / 1e6, 1)
            r["d2d_copy_GBps"] = round(nbytes / r["d2d_copy"]["median_ms"] / 1e6, 1)
            r["share_of_copy"] = round(r["d2d_copy"]["median_ms"] / r["board_tensor"]["median_ms"], 3)
            emit("board", size=N, dtype=str(dtype), **r)
            del src, dst
            if N <= 8192 and dtype == torch.uint8:
                assert np.array_equal(out.cpu().numpy(), sim.board())
            del out
    if "load" in sections:
        cells = sim.board()
        t = torch.from_numpy(cells).to(DEV)
        r = interleaved({"set_board": lambda: sim.set_board(cells), "load_tensor": lambda: sim.load_tensor(t)})
        assert np.array_equal(sim.board(), cells)
        emit("load", size=N, dtype="torch.uint8", **r)


def film_section(N, rect, n):
    kw = dict(backend="hip", device=0, rule=a.rule, film=rect)
    old = gol_amd.Simulation(N, **kw).init(5, seed=1)
    new = gol_amd.Simulation(N, **kw).init(5, seed=1)
    out = torch.empty((n,) + rect[2:], dtype=torch.uint8, device=DEV)
    got = []

    def old_way():
        old.step(n)
        got[:] = [old.film()[1]]

    r = interleaved(
        {"step_then_film": old_way, "step_film": lambda: new.step_film(n, out=out), "step_alone": lambda: old.step(n)},
        before={"step_then_film": old.film_clear, "step_alone": old.film_clear})
    old.film_clear()
    for k in list(r):
        r[k]["us_per_gen"] = round(r[k]["median_ms"] * 1e3 / n, 3)
    emit("film", size=N, window=list(rect), gens=n, kernel=new.stats()["kernel"], **r)


def soups_section():
    b = gol_amd.SoupBatch(a.soups, 64, rule=a.rule, backend="hip", seed=1)
    b.step(10)
    b.synchronize()
    out = torch.empty((a.soups, 64, 64), dtype=torch.uint8, device=DEV)
    got = []
    r = interleaved({"boards": lambda: got.__setitem__(slice(None), [b.boards()]), "boards_tensor": lambda: b.boards_tensor(out=out)})
    assert np.array_equal(out.cpu().numpy(), got[0])
    emit("soups", n=a.soups, size=64, **r)


def evolve_section():
    import torch.nn.functional as F

    from gol_amd.ops.oracle import NEIGHBOURHOODS, parse_rule_nbhd

    gens, cg = 1000, a.conv_gens
    x = (torch.rand((a.soups, 64, 64), device=DEV) < 0.5).to(torch.uint8)
    birth, survive, nbhd = parse_rule_nbhd(a.rule)
    k = torch.tensor(NEIGHBOURHOODS[nbhd], dtype=torch.float32, device=DEV)[None, None]
    lut = torch.tensor([(birth >> c) & 1 for c in range(9)] + [(survive >> c) & 1 for c in range(9)], dtype=torch.float32, device=DEV)

    def conv(g):
        y = x.to(torch.float32)[:, None]
        for _ in range(g):
            n = F.conv2d(F.pad(y, (1, 1, 1, 1), mode="circular"), k)
            y = lut[(y * 9 + n).to(torch.int64)]
        return y[:, 0].to(torch.uint8)

    assert torch.equal(gol_amd.ops.evolve(x, cg, rule=a.rule), conv(cg))
    r = interleaved({"conv2d_loop": lambda: conv(cg), "evolve": lambda: gol_amd.ops.evolve(x, gens, rule=a.rule)})
    r["conv2d_loop"]["gens"] = cg
    r["conv2d_loop"]["scaled_ms"] = round(r["conv2d_loop"]["median_ms"] * gens / cg, 2)
    r["evolve"]["gens"] = gens
    emit("evolve", shape=[a.soups, 64, 64], dtype="torch.uint8", **r)


def main():
    sections = a.sections.split(",")
    emit("setup", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, rule=a.rule)
    for N in [int(s) for s in a.sizes.split(",")]:
        if "board" in sections or "load" in sections:
            board_sections(N, sections)
    if "film" in sections:
        film_section(8192, (1000, 1000, 512, 512), 1000)
        film_section(8192, (1000, 1000, 2048, 2048), a.film_gens)
    if "soups" in sections:
        soups_section()
    if "evolve" in sections:
        evolve_section()


if __name__ == "__main__":
    main()
