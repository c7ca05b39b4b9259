"""Times pattern matching on the device against the host route (docs/PERFORMANCE.md, "Pattern matching"):
count_matches(glider, orientations="all") and match() on a pattern-5 board after 64 generations, against board() alone and
board() followed by ops.numpy_match; and SoupBatch.match_counts() of four patterns against boards() plus the oracle.
Medians of --reps rounds; within a round the legs run one after another (interleaved), each bracketed by synchronize().
The numpy legs take seconds to minutes, so they have a round count of their own.  The first device call after board() or
boards() pays 4 to 11 ms here whatever it is (population() too), so an untimed device call follows those legs.

    python tools/measure_match.py [--sizes 8192,32768] [--reps 5] [--oracle-reps 1] [--soups 16384] [--json out.json]
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
from gol_amd.ops import match_template, numpy_match  # noqa: E402

GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)
BLOCK = np.ones((2, 2), dtype=np.uint8)
BLINKER = np.ones((1, 3), dtype=np.uint8)
BEEHIVE = np.array([[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0]], dtype=np.uint8)


def rounds(legs, reps, sync):
    """{name: [ms, ...]}: `reps` rounds over the legs (name, fn, every, after), a leg with every = k running in rounds
    0, k, 2k ...; `after` (or None) runs untimed behind the leg."""
    out = {leg[0]: [] for leg in legs}
    for i in range(reps):
        for name, fn, every, after in legs:
            if i % every:
                continue
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            out[name].append((time.perf_counter() - t0) * 1e3)
            if after:
                after()
    return out


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def measure_board(N, reps, oracle_reps):
    sim = gol_amd.Simulation(N, backend="hip", device=0).init(5, seed=1)
    sim.step(64)
    t = match_template(GLIDER)
    sim.count_matches(t, orientations="all")  # (warm-up: the bitmap-free path)
    sim.match(t, orientations="all")          # (the bitmap and the position buffers)
    keep = {}

    def host():
        keep["host"] = numpy_match(sim.board(), t, "torus", "all")

    def device():
        keep["device"] = sim.match(t, orientations="all")

    legs = [
        ("count_matches", lambda: sim.count_matches(t, orientations="all"), 1, None),
        ("match", device, 1, None),
        ("match_tensor", lambda: sim.match_tensor(t, orientations="all"), 1, None),
        ("board", sim.board, 1, sim.population),
        ("board+numpy_match", host, max(1, reps // max(1, oracle_reps)), sim.population),
    ]
    res = {k: summary(v) for k, v in rounds(legs, reps, sim.synchronize).items()}
    pos, ids = keep["host"]
    assert keep["device"].count == len(pos) and np.array_equal(keep["device"].positions, pos)
    assert np.array_equal(keep["device"].orientation, ids)
    res["size"], res["gliders"], res["kernel"] = N, len(pos), sim.stats()["kernel"]
    return res


def measure_soups(n, reps, oracle_reps):
    batch = gol_amd.SoupBatch(n, 64, backend="hip", seed=0)
    batch.settle(200)
    patterns = [BLOCK, BLINKER, BEEHIVE, GLIDER]
    templates = [match_template(p) for p in patterns]
    batch.match_counts(templates)
    keep = {}

    def host():
        boards = batch.boards()
        out = np.zeros((n, len(templates)), dtype=np.uint32)
        for i in range(n):
            for k, t in enumerate(templates):
                out[i, k] = len(numpy_match(boards[i], t, "torus", "all")[0])
        keep["host"] = out

    def device():
        keep["device"] = batch.match_counts(templates)

    settle = lambda: batch.match_counts(templates[:1])  # noqa: E731  (untimed, behind the legs that read the boards)
    legs = [("match_counts", device, 1, None), ("boards", batch.boards, 1, settle),
            ("boards+numpy_match", host, max(1, reps // max(1, oracle_reps)), settle)]
    res = {k: summary(v) for k, v in rounds(legs, reps, batch.synchronize).items()}
    assert np.array_equal(keep["device"], keep["host"])
    res["soups"], res["totals"] = n, [int(v) for v in keep["device"].sum(axis=0)]
    return res


def show(title, res):
    print(title)
    for k, v in res.items():
        if isinstance(v, dict):
            print(f"  {k:20s} median {v['median_ms']:12.3f} ms   min {v['min_ms']:12.3f}   max {v['max_ms']:12.3f}   n {v['n']}", flush=True)
        else:
            print(f"  {k:20s} {v}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-reps", type=int, default=1, help="rounds in which the numpy legs run")
    ap.add_argument("--soups", type=int, default=16384, help="0: skip the soup batch")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = {"boards": [], "reps": a.reps}
    for N in [int(v) for v in a.sizes.split(",") if v]:
        out["boards"].append(measure_board(N, a.reps, a.oracle_reps))
        show(f"board {N} x {N}", out["boards"][-1])
    if a.soups:
        out["soups"] = measure_soups(a.soups, a.reps, a.oracle_reps)
        show(f"{a.soups} soups of 64 x 64", out["soups"])
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
