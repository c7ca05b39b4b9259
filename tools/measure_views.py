"""Times the views and pattern I/O of a live board against the whole-board readers (docs/PERFORMANCE.md,
"Views and pattern I/O"): density(64), density(512), a 1024 x 1024 window() and stamp(), population() and
board() on one GPU after init(5).  Median of --reps calls after --warmup calls, each bracketed by synchronize().

    python tools/measure_views.py [--size 32768] [--reps 10] [--warmup 2] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gol_amd  # noqa: E402


def timed(sim, fn, reps, warmup):
    ts = []
    for i in range(warmup + reps):
        sim.synchronize()
        t0 = time.perf_counter()
        fn()
        sim.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--board-reps", type=int, default=10, help="calls of board(), seconds each on a big board")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    N = a.size
    sim = gol_amd.Simulation(N, backend="hip", device=0).init(5, seed=1)
    sim.step(64)
    side = min(1024, N)
    pat = gol_amd.ops.pattern_from_cells((np.random.default_rng(1).random((side, side)) < 0.3).astype(np.uint8))
    res = {"size": N, "kernel": sim.stats()["kernel"], "reps": a.reps, "warmup": a.warmup}
    res["population"] = timed(sim, sim.population, a.reps, a.warmup)
    res["density_64"] = timed(sim, lambda: sim.density(64), a.reps, a.warmup)
    res["density_512"] = timed(sim, lambda: sim.density(512), a.reps, a.warmup)
    res["density_1x64"] = timed(sim, lambda: sim.density(1, 64), a.reps, a.warmup)
    res["window_aligned"] = timed(sim, lambda: sim.window(1024, 1024, side, side), a.reps, a.warmup)
    res["window_unaligned"] = timed(sim, lambda: sim.window(N - 500, N - 500, side, side), a.reps, a.warmup)
    res["stamp_aligned"] = timed(sim, lambda: sim.stamp(pat, at=(1024, 1024), mode="xor"), a.reps, a.warmup)
    res["stamp_unaligned"] = timed(sim, lambda: sim.stamp(pat, at=(N - 500, N - 500), mode="xor"), a.reps, a.warmup)
    res["board"] = timed(sim, sim.board, a.board_reps, min(a.warmup, 1))
    # consistency: the views agree with the whole-board readers on this board
    b = sim.board()
    assert int(sim.density(512).sum()) == int(b.sum()) == sim.population()
    assert np.array_equal(sim.window(N - 500, N - 500, side, side),
                          np.take(np.take(b, np.arange(N - 500, N - 500 + side), 0, mode="wrap"),
                                  np.arange(N - 500, N - 500 + side), 1, mode="wrap"))
    for k, v in res.items():
        if isinstance(v, dict):
            print(f"{k:18s} median {v['median_ms']:10.3f} ms   min {v['min_ms']:10.3f}   max {v['max_ms']:10.3f}")
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
