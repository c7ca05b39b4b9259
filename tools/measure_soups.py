"""Times soup batches (docs/PERFORMANCE.md section 27) on one GPU against the loop they replace:

  step    SoupBatch(n, S, rule).step(g), synchronised: soups x generations per second and cell updates per second
  settle  SoupBatch(n, 64).settle(max_gens) on seeds seed .. seed + n - 1, construction and init untimed
  loop    the only way before: one Simulation(S, backend="hip") per soup; step(g) per soup, and
          Simulation(64, signature=True).find_cycle(max_gens) per soup (engine construction and init untimed), over a
          sample of --sample soups, scaled per soup

The batch and the loop are timed interleaved, rep by rep, on the same box.  Median, min and max of --reps timed
calls after --warmup calls.

    python tools/measure_soups.py [--n 16384] [--gens 32768] [--loop-gens 4096] [--max-gens 20000] [--sample 32] [--reps 5] [--workgroup 256]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--gens", type=int, default=32768, help="generations of a timed batch step()")
ap.add_argument("--loop-gens", type=int, default=4096, help="generations of a timed step() of each soup of the loop")
ap.add_argument("--max-gens", type=int, default=20000)
ap.add_argument("--sample", type=int, default=32)
ap.add_argument("--seed", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--workgroup", type=int, default=0)
ap.add_argument("--sizes", default="64,128")
ap.add_argument("--rules", default="B3/S23,B36/S23")
ap.add_argument("--skip-loop", action="store_true")
ap.add_argument("--skip-settle", action="store_true")
ap.add_argument("--backend", default="hip")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gol_amd  # noqa: E402


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "all_ms": [round(t, 3) for t in ts]}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure_step(S, rule):
    n, g = a.n, a.gens
    sb = gol_amd.SoupBatch(n, S, rule, backend=a.backend, seed=a.seed, workgroup=a.workgroup)
    sims = []
    if not a.skip_loop:
        sims = [gol_amd.Simulation(S, backend=a.backend, rule=rule).init(5, seed=a.seed + i) for i in range(a.sample)]

    def batch():
        sb.step(g)
        sb.synchronize()

    def loop():
        for s in sims:
            s.step(a.loop_gens)
        for s in sims:
            s.synchronize()

    tb, tl = [], []
    for i in range(a.warmup + a.reps):  # interleaved
        b = clock(batch)
        l = clock(loop) if sims else 0.0
        if i >= a.warmup:
            tb.append(b)
            tl.append(l)
    r = {"size": S, "rule": rule, "n": n, "gens": g, "kernel": sb.stats()["kernel"], "workgroup": sb.stats()["workgroup"],
         "batch": summary(tb)}
    sec = r["batch"]["median_ms"] * 1e-3
    r["batch"]["soup_gens_per_s"] = n * g / sec
    r["batch"]["cell_updates_per_s"] = n * g * S * S / sec
    if sims:
        r["loop"] = summary(tl)
        r["loop"]["sample"] = a.sample
        r["loop"]["kernel"] = sims[0].stats()["kernel"]
        lsec = r["loop"]["median_ms"] * 1e-3
        r["loop"]["gens"] = a.loop_gens
        r["loop"]["soup_gens_per_s"] = a.sample * a.loop_gens / lsec
        r["loop"]["cell_updates_per_s"] = a.sample * a.loop_gens * S * S / lsec
        r["batch_over_loop"] = r["batch"]["soup_gens_per_s"] / r["loop"]["soup_gens_per_s"]
    return r


def measure_settle():
    n, S = a.n, 64
    tb, tl = [], []
    out = {"size": S, "rule": "B3/S23", "n": n, "max_gens": a.max_gens, "seed": a.seed}
    for i in range(a.warmup + a.reps):
        sb = gol_amd.SoupBatch(n, S, backend=a.backend, seed=a.seed, workgroup=a.workgroup)  # (untimed)
        res = []
        b = clock(lambda: res.append(sb.settle(a.max_gens)))
        out["settled"] = int((res[0].period > 0).sum())
        out["launches"] = sb.stats()["launches"]
        l = 0.0
        if not a.skip_loop:
            sims = [gol_amd.Simulation(S, backend=a.backend, signature=True).init(5, seed=a.seed + k) for k in range(a.sample)]
            cyc = []
            l = clock(lambda: cyc.extend(s.find_cycle(a.max_gens) for s in sims))
            # the same soups: the loop's periods are the batch's
            assert [c.period if c else 0 for c in cyc] == [int(p) for p in res[0].period[: a.sample]]
            del sims
        if i >= a.warmup:
            tb.append(b)
            tl.append(l)
    out["batch"] = summary(tb)
    out["batch"]["ms_per_soup"] = out["batch"]["median_ms"] / n
    if not a.skip_loop:
        out["loop"] = summary(tl)
        out["loop"]["sample"] = a.sample
        out["loop"]["ms_per_soup"] = out["loop"]["median_ms"] / a.sample
        out["loop_over_batch_per_soup"] = out["loop"]["ms_per_soup"] / out["batch"]["ms_per_soup"]
    return out


def main():
    res = {"reps": a.reps, "warmup": a.warmup, "step": []}
    for S in (int(v) for v in a.sizes.split(",")):
        for rule in a.rules.split(","):
            res["step"].append(measure_step(S, rule))
            print(json.dumps(res["step"][-1]), flush=True)
    if not a.skip_settle:
        res["settle"] = measure_settle()
        print(json.dumps(res["settle"]), flush=True)


if __name__ == "__main__":
    main()
