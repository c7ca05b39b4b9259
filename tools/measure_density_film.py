"""Times the density maps of the whole board over a run, counted inside the kernel (density-film mode) against the loop
it replaces (docs/PERFORMANCE.md, "Density-film mode"), on one GPU after init(5), rule B36/S23:

  new     Simulation(density_film=blocks): step(n), then one density_film() call (maps on the host;
          density_film_clear() before, untimed)
  pass    the same step(n) alone, synchronised: us per generation of density@D (the maps stay on the device)
  census  a census simulation at the same explicit pass depth: step(n), us per generation of census@D
  rule    a plain simulation at the same explicit pass depth: step(n), us per generation of rule@D
  old     the plain simulation's  for g in range(n): step(1); density(*blocks)

Median, min and max of --reps timed calls after --warmup calls.

    python tools/measure_density_film.py --size 8192 --gens 1000 --blocks 512 [--boundary dead] [--depth 8] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=8192)
ap.add_argument("--gens", type=int, default=1000)
ap.add_argument("--blocks", type=int, default=512, help="side of the square blocks (a multiple of 64)")
ap.add_argument("--boundary", default="torus")
ap.add_argument("--rule", default="B36/S23")
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--skip-old", action="store_true")
ap.add_argument("--backend", default="hip")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gol_amd  # noqa: E402
import numpy as np  # noqa: E402


def timed(fn, sync, before=None):
    ts = []
    for i in range(a.warmup + a.reps):
        if before:
            before()  # (untimed)
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= a.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "all_ms": [round(t, 3) for t in ts]}


def per_gen(r, n):
    r["us_per_gen"] = r["median_ms"] * 1e3 / n
    return r


def main():
    N, n, b = a.size, a.gens, a.blocks
    blocks = (b, b)
    kw = dict(backend=a.backend, boundary=a.boundary, kernel_depth=a.depth, rule=a.rule)
    if a.backend == "hip":
        kw["device"] = 0
    res = {"size": N, "gens": n, "blocks": list(blocks), "boundary": a.boundary, "rule_name": a.rule, "depth": a.depth, "reps": a.reps}
    sim = gol_amd.Simulation(N, density_film=blocks, **kw).init(5, seed=1)
    res["density_kernel"] = sim.stats()["kernel"]
    got = []

    def new_way():
        sim.step(n)
        got[:] = [sim.density_film()]

    res["new"] = timed(new_way, sim.synchronize, before=sim.density_film_clear)
    maps = got[0][1]
    assert maps.shape == (n, -(-N // b), -(-N // b)) and np.array_equal(maps[-1], sim.density(*blocks))

    res["pass"] = per_gen(timed(lambda: sim.step(n), sim.synchronize, before=sim.density_film_clear), n)
    sim.density_film_clear()
    del sim, maps, got
    census = gol_amd.Simulation(N, census=True, **kw).init(5, seed=1)
    res["census_kernel"] = census.stats()["kernel"]
    res["census"] = per_gen(timed(lambda: census.step(n), census.synchronize, before=census.census_clear), n)
    del census
    plain = gol_amd.Simulation(N, **kw).init(5, seed=1)
    res["rule_kernel"] = plain.stats()["kernel"]
    res["rule"] = per_gen(timed(lambda: plain.step(n), plain.synchronize), n)
    if not a.skip_old:
        loop = []

        def old_way():
            loop.clear()
            for _ in range(n):
                plain.step(1)
                loop.append(plain.density(*blocks))

        res["old"] = timed(old_way, plain.synchronize)
        assert len(loop) == n
        res["old_over_new"] = res["old"]["median_ms"] / res["new"]["median_ms"]
    res["density_over_census"] = res["pass"]["us_per_gen"] / res["census"]["us_per_gen"]
    res["density_over_rule"] = res["pass"]["us_per_gen"] / res["rule"]["us_per_gen"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
