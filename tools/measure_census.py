"""Times the population series of a run, counted inside the kernel (census mode) against the loop it replaces
(docs/PERFORMANCE.md, "Population census"), on one GPU after init(5), rule B36/S23:

  new    Simulation(census=True): step(n) then census()                      (trees that have census mode)
  pass   the same step(n) alone, synchronised: us per generation of census@D
  rule   a plain simulation at the same explicit pass depth: step(n), us per generation of rule@D (graph replays),
         and the same with graph=False (rule_eager: eager launches, as census runs are)
  old    the plain simulation's  for g in range(n): step(1); population()

Median, min and max of --reps timed calls after --warmup calls.  --tree names the checkout whose package is
imported (default: this one), so the same tool times a build of the parent commit; such a tree has no census mode
and reports rule and old alone.

    python tools/measure_census.py --size 8192 --gens 1000 [--boundary dead] [--depth 8] [--reps 5] [--tree DIR]
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
ap.add_argument("--depth", type=int, default=0, help="pass depth (0: the census kernel's deepest, else 8)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--skip-old", action="store_true")
ap.add_argument("--backend", default="hip")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
import gol_amd  # noqa: E402


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


def main():
    N, n = a.size, a.gens
    has_census = "census" in inspect.signature(gol_amd.Simulation.__init__).parameters
    depth = a.depth or (gol_amd.native.max_census_depth() if has_census else 8)
    res = {"tree": os.path.abspath(a.tree), "size": N, "gens": n, "boundary": a.boundary, "rule_name": a.rule, "depth": depth,
           "reps": a.reps}
    kw = dict(backend=a.backend, rule=a.rule, boundary=a.boundary, kernel_depth=depth)
    if a.backend == "hip":
        kw["device"] = 0
    if has_census:
        sim = gol_amd.Simulation(N, census=True, **kw).init(5, seed=1)
        res["census_kernel"] = sim.stats()["kernel"]
        series = []

        def new_way():
            sim.census_clear()
            sim.step(n)
            series[:] = [sim.census()[1]]

        res["new"] = timed(new_way, sim.synchronize)
        assert len(series[0]) == n and int(series[0][-1]) == sim.population()
        res["pass"] = timed(lambda: sim.step(n), sim.synchronize)
        res["pass"]["us_per_gen"] = res["pass"]["median_ms"] * 1e3 / n
        sim.census_clear()
        del sim
    plain = gol_amd.Simulation(N, **kw).init(5, seed=1)
    res["rule_kernel"] = plain.stats()["kernel"]
    res["rule"] = timed(lambda: plain.step(n), plain.synchronize)
    res["rule"]["us_per_gen"] = res["rule"]["median_ms"] * 1e3 / n
    eager = gol_amd.Simulation(N, graph=False, **kw).init(5, seed=1)  # census runs are eager: what the graphs are worth
    res["rule_eager"] = timed(lambda: eager.step(n), eager.synchronize)
    res["rule_eager"]["us_per_gen"] = res["rule_eager"]["median_ms"] * 1e3 / n
    del eager
    if not a.skip_old:
        pops = []

        def old_way():
            pops.clear()
            for _ in range(n):
                plain.step(1)
                pops.append(plain.population())

        res["old"] = timed(old_way, plain.synchronize)
        assert len(pops) == n
    if "new" in res and "old" in res:
        res["old_over_new"] = res["old"]["median_ms"] / res["new"]["median_ms"]
    if "pass" in res:
        res["census_over_rule"] = res["pass"]["us_per_gen"] / res["rule"]["us_per_gen"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
