"""Times the envelope of a run, ORed inside the kernel (envelope mode) against the loop it replaces
(docs/PERFORMANCE.md, "Envelope mode"), on one GPU after init(5), rule B36/S23:

  new     Simulation(envelope=True): step(n), then one envelope() call (the cells on the host; envelope_clear()
          before, untimed)
  pass    the same step(n) alone, synchronised: us per generation of envelope@D (the envelope stays on the device)
  rule    a plain simulation at the same explicit pass depth: step(n), us per generation of rule@D
  old     the plain simulation's  for g in range(m): step(1); env |= board()  over m = --old-gens generations (the
          whole board crosses to the host every generation), scaled to n generations as old_scaled_ms

Median, min and max of --reps timed calls after --warmup calls.  (envelope@D against the rule@D of another commit:
run this tool with --skip-old in a build of that commit's tree too; it then times rule only.)

    python tools/measure_envelope.py --size 8192 --gens 1000 [--boundary dead] [--depth 8] [--reps 5] [--old-gens 20]
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
ap.add_argument("--old-gens", type=int, default=20, help="generations of the host loop (its time is scaled to --gens)")
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


def timed(fn, sync, before=None, reps=None):
    ts = []
    reps = reps or a.reps
    for i in range(a.warmup + reps):
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
    N, n, m = a.size, a.gens, a.old_gens
    kw = dict(backend=a.backend, boundary=a.boundary, kernel_depth=a.depth, rule=a.rule)
    if a.backend == "hip":
        kw["device"] = 0
    res = {"size": N, "gens": n, "boundary": a.boundary, "rule_name": a.rule, "depth": a.depth, "reps": a.reps}
    if "envelope" in gol_amd.Simulation.__init__.__code__.co_varnames:  # (a tree from before the mode times rule only)
        sim = gol_amd.Simulation(N, envelope=True, **kw).init(5, seed=1)
        res["envelope_kernel"] = sim.stats()["kernel"]
        got = []

        def new_way():
            sim.step(n)
            got[:] = [sim.envelope()]

        res["new"] = timed(new_way, sim.synchronize, before=sim.envelope_clear)
        start, cells = got[0]
        assert cells.shape == (N, N) and start == sim.generation - n and not (sim.board() & ~cells).any()
        res["envelope_cells"] = int(cells.sum())
        res["pass"] = per_gen(timed(lambda: sim.step(n), sim.synchronize, before=sim.envelope_clear), n)
        del sim, cells, got
    plain = gol_amd.Simulation(N, **kw).init(5, seed=1)
    res["rule_kernel"] = plain.stats()["kernel"]
    res["rule"] = per_gen(timed(lambda: plain.step(n), plain.synchronize), n)
    if not a.skip_old:
        env = [None]

        def old_way():
            e = plain.board()
            for _ in range(m):
                plain.step(1)
                e |= plain.board()
            env[0] = e

        res["old"] = timed(old_way, plain.synchronize, reps=min(a.reps, 3))
        res["old"]["gens"] = m
        res["old_scaled_ms"] = res["old"]["median_ms"] * n / m
        if "new" in res:
            res["old_over_new"] = res["old_scaled_ms"] / res["new"]["median_ms"]
    if "pass" in res:
        res["envelope_over_rule"] = res["pass"]["us_per_gen"] / res["rule"]["us_per_gen"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
