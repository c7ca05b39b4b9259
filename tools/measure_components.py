"""Times connected components on the device against the host route (docs/PERFORMANCE.md, "Connected components"):
count_components(), components() with and without hashes and components_tensor() on a pattern-5 board in two states --
the raw density-0.5 board (one giant component: the worst case for the atomics) and the ash after the population has gone
flat -- against board() alone and board() followed by a host labeller (scipy.ndimage.label where it imports, else
ops.numpy_components; scipy labels the bounded board, which is the same work); and SoupBatch.components() of settled soups
against boards() alone.  On the raw board the records are also timed with native.cc_wave_reduce(False) (no reduction
across a wave before the atomics of k_cc_stats / k_cc_hash).  Medians of --reps rounds after one warm-up; within a round the legs
run one after another (interleaved), each bracketed by synchronize().  The host labeller has a round count of its own.
The first device call after board() or boards() pays a few ms whatever it is, so an untimed device call follows those legs.

    python tools/measure_components.py [--sizes 8192,32768] [--reps 5] [--host-reps 1] [--soups 16384] [--json out.json]
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
from gol_amd.ops import numpy_components  # noqa: E402

try:
    from scipy import ndimage
except ImportError:  # (the numpy oracle then stands in)
    ndimage = None


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


def host_label(board):
    if ndimage is not None:
        return int(ndimage.label(board, structure=np.ones((3, 3), int))[1])
    return numpy_components(board, "moore", "torus")[1].count


def settle(sim, chunk, max_gens):
    """Steps until the population moves by less than 0.1 % over a chunk (or max_gens); (generations, population, flat)."""
    gens, last = 0, sim.population()
    while gens < max_gens:
        sim.step(chunk)
        gens += chunk
        now = sim.population()
        if abs(now - last) <= last // 1000:
            return gens, now, True
        last = now
    return gens, last, False


def measure_state(sim, state, reps, host_reps, wave_switch):
    def without_reduce():
        gol_amd.native.cc_wave_reduce(False)
        try:
            sim.components()
        finally:
            gol_amd.native.cc_wave_reduce(True)

    keep = {}

    def device():
        keep["device"] = sim.components()

    def host():
        keep["host"] = host_label(sim.board())

    for warm in (sim.count_components, sim.components, sim.components_tensor):
        warm()
    legs = [
        ("count_components", sim.count_components, 1, None),
        ("components(hashes=False)", lambda: sim.components(hashes=False), 1, None),
        ("components", device, 1, None),
        ("components_tensor", sim.components_tensor, 1, None),
        ("board", sim.board, 1, sim.population),
        ("board+host_labeller", host, max(1, reps // max(1, host_reps)), sim.population),
    ]
    if wave_switch:
        legs.insert(3, ("components, no wave reduce", without_reduce, 1, None))
    res = {k: summary(v) for k, v in rounds(legs, reps, sim.synchronize).items()}
    d = keep["device"]
    res["state"], res["objects"], res["truncated"] = state, d.count, d.truncated
    res["largest"] = int(d.population.max()) if len(d.population) else 0
    res["distinct_hashes"] = int(len(np.unique(d.hash)))
    res["host_objects_bounded"] = keep["host"]
    return res


def measure_board(N, reps, host_reps, chunk, max_gens):
    sim = gol_amd.Simulation(N, backend="hip", device=0).init(5, seed=1)
    out = {"size": N, "parent_bytes": 4 * N * N, "host_labeller": "scipy.ndimage.label" if ndimage is not None else "ops.numpy_components"}
    out["raw"] = measure_state(sim, "raw density 0.5", reps, host_reps, True)
    gens, pop, flat = settle(sim, chunk, max_gens)
    out["ash"] = measure_state(sim, f"after {gens} generations (population {pop}, flat: {flat})", reps, host_reps, False)
    return out


def measure_soups(n, reps):
    batch = gol_amd.SoupBatch(n, 64, backend="hip", seed=0)
    rec = batch.settle(20000)
    batch.components()
    keep = {}

    def device():
        keep["device"] = batch.components()

    after = lambda: batch.component_counts()  # noqa: E731  (untimed, behind the leg that reads the boards)
    legs = [("component_counts", batch.component_counts, 1, None), ("components", device, 1, None),
            ("components(hashes=False)", lambda: batch.components(hashes=False), 1, None), ("boards", batch.boards, 1, after)]
    res = {k: summary(v) for k, v in rounds(legs, reps, batch.synchronize).items()}
    res["soups"], res["settled"], res["objects"] = n, int((rec.period != 0).sum()), keep["device"].count
    res["distinct_hashes"] = int(len(np.unique(keep["device"].hash)))
    return res


def show(title, res):
    print(title)
    for k, v in res.items():
        if isinstance(v, dict) and "median_ms" in v:
            print(f"  {k:28s} median {v['median_ms']:12.3f} ms   min {v['min_ms']:12.3f}   max {v['max_ms']:12.3f}   n {v['n']}", flush=True)
        elif isinstance(v, dict):
            show(f" {title}: {k}", v)
        else:
            print(f"  {k:28s} {v}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1, help="rounds in which the host labeller runs")
    ap.add_argument("--chunk", type=int, default=1024, help="generations between two looks at the population")
    ap.add_argument("--max-gens", type=int, default=16384)
    ap.add_argument("--soups", type=int, default=16384, help="0: skip the soup batch")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = {"boards": [], "reps": a.reps}
    for N in [int(v) for v in a.sizes.split(",") if v]:
        out["boards"].append(measure_board(N, a.reps, a.host_reps, a.chunk, a.max_gens))
        show(f"board {N} x {N}", out["boards"][-1])
    if a.soups:
        out["soups"] = measure_soups(a.soups, a.reps)
        show(f"{a.soups} soups of 64 x 64", out["soups"])
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
