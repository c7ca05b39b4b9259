"""Times the signature series of a run, hashed inside the kernel (signature mode) against the loop it replaces
(docs/PERFORMANCE.md, "Signature mode"), on one GPU after init(5), rule B36/S23:

  new     Simulation(signature=True): step(n) then signatures()                (trees that have signature mode)
  pass    the same step(n) alone, synchronised: us per generation of sig@D
  census  Simulation(census=True) at the same pass depth: step(n), us per generation of census@D
  rule    a plain simulation at the same explicit pass depth: step(n), us per generation of rule@D
  old     the plain simulation's  for g in range(n): step(1); fingerprint()

Median, min and max of --reps timed calls after --warmup calls.  --tree names the checkout whose package is
imported (default: this one), so the same tool times a build of the parent commit; such a tree has no signature
mode and reports census, rule and old alone.

--find-cycle times, once, find_cycle(--max-generations, chunk=256) on the R-pentomino at the centre of a
--size torus (B3/S23), or on a tree without it the same search done with step(1); fingerprint() and a dict.

    python tools/measure_signature.py --size 8192 --gens 1000 [--boundary dead] [--depth 8] [--reps 5] [--tree DIR]
    python tools/measure_signature.py --size 4096 --find-cycle [--tree DIR]
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=8192)
ap.add_argument("--gens", type=int, default=1000)
ap.add_argument("--boundary", default="torus")
ap.add_argument("--rule", default="B36/S23")
ap.add_argument("--depth", type=int, default=0, help="pass depth (0: the signature kernel's deepest, else 8)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--skip-old", action="store_true")
ap.add_argument("--find-cycle", action="store_true")
ap.add_argument("--max-generations", type=int, default=20000)
ap.add_argument("--backend", default="hip")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
import gol_amd  # noqa: E402
import numpy as np  # noqa: E402


def timed(fn, sync):
    ts = []
    for i in range(a.warmup + a.reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= a.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def per_gen(r, n):
    r["us_per_gen"] = r["median_ms"] * 1e3 / n
    return r


def find_cycle(has_signature, kw):
    N = a.size
    pent = np.array([[0, 1, 1], [1, 1, 0], [0, 1, 0]], np.uint8)
    res = {"tree": os.path.abspath(a.tree), "size": N, "max_generations": a.max_generations}
    if has_signature:
        sim = gol_amd.Simulation(N, signature=True, **kw).init(0)
        sim.stamp(pent, at="center")
        sim.synchronize()
        t0 = time.perf_counter()
        c = sim.find_cycle(a.max_generations, chunk=256)
        res["find_cycle_ms"] = (time.perf_counter() - t0) * 1e3
        res["result"] = None if c is None else list(c)
    else:
        sim = gol_amd.Simulation(N, **kw).init(0)
        sim.stamp(pent, at="center")
        sim.synchronize()
        t0 = time.perf_counter()
        seen, hit = {sim.fingerprint(): 0}, None
        for g in range(1, a.max_generations + 1):
            sim.step(1)
            f = sim.fingerprint()
            if f in seen:
                hit = (seen[f], g - seen[f], g, sim.population())
                break
            seen[f] = g
        res["old_search_ms"] = (time.perf_counter() - t0) * 1e3
        res["result"] = None if hit is None else list(hit)
    print(json.dumps(res))


def main():
    N, n = a.size, a.gens
    params = inspect.signature(gol_amd.Simulation.__init__).parameters
    has_signature, has_census = "signature" in params, "census" in params
    depth = a.depth or (gol_amd.native.max_signature_depth() if has_signature else 8)
    kw = dict(backend=a.backend, boundary=a.boundary, kernel_depth=depth)
    if a.backend == "hip":
        kw["device"] = 0
    if a.find_cycle:
        return find_cycle(has_signature, dict(kw, rule="B3/S23"))
    kw["rule"] = a.rule
    res = {"tree": os.path.abspath(a.tree), "size": N, "gens": n, "boundary": a.boundary, "rule_name": a.rule, "depth": depth,
           "reps": a.reps}
    if has_signature:
        sim = gol_amd.Simulation(N, signature=True, **kw).init(5, seed=1)
        res["signature_kernel"] = sim.stats()["kernel"]
        series = []

        def new_way():
            sim.signatures_clear()
            sim.step(n)
            series[:] = [sim.signatures()]

        res["new"] = timed(new_way, sim.synchronize)
        assert len(series[0][1]) == n and int(series[0][1][-1]) == sim.signature() and int(series[0][2][-1]) == sim.population()
        res["pass"] = per_gen(timed(lambda: sim.step(n), sim.synchronize), n)
        sim.signatures_clear()
        del sim
    if has_census:
        cs = gol_amd.Simulation(N, census=True, **kw).init(5, seed=1)
        res["census_kernel"] = cs.stats()["kernel"]
        res["census"] = per_gen(timed(lambda: cs.step(n), cs.synchronize), n)
        cs.census_clear()
        del cs
    plain = gol_amd.Simulation(N, **kw).init(5, seed=1)
    res["rule_kernel"] = plain.stats()["kernel"]
    res["rule"] = per_gen(timed(lambda: plain.step(n), plain.synchronize), n)
    if not a.skip_old:
        prints = []

        def old_way():
            prints.clear()
            for _ in range(n):
                plain.step(1)
                prints.append(plain.fingerprint())

        res["old"] = timed(old_way, plain.synchronize)
        assert len(prints) == n
    if "new" in res and "old" in res:
        res["old_over_new"] = res["old"]["median_ms"] / res["new"]["median_ms"]
    if "pass" in res:
        res["sig_over_rule"] = res["pass"]["us_per_gen"] / res["rule"]["us_per_gen"]
        if "census" in res:
            res["sig_over_census"] = res["pass"]["us_per_gen"] / res["census"]["us_per_gen"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
