"""Times the Larger than Life kernel step_ltl (docs/PERFORMANCE.md section 32) on one GPU, at each of --sizes:

  ltl@1 R1    Simulation(rule="R1,C0,M0,S2..3,B3..3,NM"): step(n), us per generation
  rule@1      B3/S23 through the generic kernel at one generation per pass (kernel="rule", kernel_depth=1, halo_depth=1):
              the same rule and the same memory traffic as the leg above
  ltl@1 R5    Bosco's rule, R5,C0,M1,S34..58,B34..45,NM
  ltl@1 R7    R7,C0,M1,S63..108,B63..84,NM
  torch R5/R7 what a user would write today: a loop over a device float32 tensor, circular padding plus avg_pool2d with
              a (2R+1)^2 box (divisor 1: the box sum), then the two interval tests; --torch-gens generations

Every leg starts from the density-gradient board of tests/ltl_cases.py (a uniform soup dies under these rules).  Every
figure is the median of --reps timed calls after one warm-up call, the legs of one size interleaved round by round in
this one process.  One JSON line per size, then a table.

    python tools/measure_ltl.py [--sizes 8192,32768] [--gens 60] [--torch-gens 4] [--reps 5] [--skip-torch]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="8192,32768")
ap.add_argument("--gens", type=int, default=60, help="generations per timed step() call")
ap.add_argument("--torch-gens", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-torch", action="store_true")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gol_amd  # noqa: E402
from gol_amd.ops import parse_ltl_rule  # noqa: E402

LIFE = "R1,C0,M0,S2..3,B3..3,NM"
BOSCO = "R5,C0,M1,S34..58,B34..45,NM"
R7 = "R7,C0,M1,S63..108,B63..84,NM"


def gradient_board(N, seed=1):
    rng = np.random.default_rng(seed)
    out = np.empty((N, N), np.uint8)
    c = np.arange(N, dtype=np.int64)[None, :]
    for r0 in range(0, N, 1024):  # (in bands: the temporaries of a 32768^2 board would take tens of GB)
        r = np.arange(r0, min(N, r0 + 1024), dtype=np.int64)[:, None]
        p = ((r + c) % N).astype(np.float32) / np.float32(N - 1)
        out[r0 : r0 + 1024] = rng.random(p.shape, dtype=np.float32) < p
    return out


def clock(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def interleaved(variants, reps):
    out = {k: [] for k in variants}
    for r in range(reps + 1):  # (round 0 warms up)
        for k, (fn, sync, _) in variants.items():
            ms = clock(fn, sync)
            if r:
                out[k].append(ms)
    return out


def torch_loop(board, rule, gens):
    import torch
    import torch.nn.functional as F

    R, M, smin, smax, bmin, bmax = parse_ltl_rule(rule)
    x = torch.as_tensor(board, device="cuda").to(torch.float32)[None, None]

    def run():
        nonlocal x
        for _ in range(gens):
            n = F.avg_pool2d(F.pad(x, (R, R, R, R), mode="circular"), 2 * R + 1, stride=1, divisor_override=1)
            if not M:
                n = n - x
            alive = x > 0.5
            x = torch.where(alive, (n >= smin - 0.5) & (n <= smax + 0.5), (n >= bmin - 0.5) & (n <= bmax + 0.5)).to(torch.float32)

    return run, torch.cuda.synchronize, (lambda: x[0, 0].to(torch.uint8).cpu().numpy())


if not a.skip_torch:  # the torch loop computes the rule: two generations at 128^2 against the numpy oracle
    from gol_amd.ops import numpy_ltl  # noqa: E402

    for rule in (BOSCO, "R7,C0,M0,S61..106,B63..84,NM"):
        run, sync, read = torch_loop(gradient_board(128), rule, 2)
        run()
        sync()
        assert np.array_equal(read(), numpy_ltl(gradient_board(128), rule, 2)), rule

rows = []
for N in [int(v) for v in a.sizes.split(",")]:
    start = gradient_board(N)
    variants = {}
    sims = {}
    for name, kw in (("ltl@1 R1", dict(rule=LIFE)), ("rule@1", dict(rule="B3/S23", kernel="rule", kernel_depth=1, halo_depth=1)),
                     ("ltl@1 R5", dict(rule=BOSCO)), ("ltl@1 R7", dict(rule=R7))):
        s = gol_amd.Simulation(N, backend="hip", device=0, run_hint=a.gens, **kw)
        s.init(0)
        s.set_board(start)
        sims[name] = s
        variants[name] = ((lambda s=s: s.step(a.gens)), s.synchronize, a.gens)
    if not a.skip_torch:
        for name, rule in (("torch R5", BOSCO), ("torch R7", R7)):
            fn, sync, _ = torch_loop(start, rule, a.torch_gens)
            variants[name] = (fn, sync, a.torch_gens)
    ms = interleaved(variants, a.reps)
    res = {"N": N, "gens": a.gens, "torch_gens": a.torch_gens, "reps": a.reps}
    for k, v in ms.items():
        g = variants[k][2]
        res[k] = {"us_per_gen": statistics.median(v) * 1e3 / g, "min_us": min(v) * 1e3 / g, "max_us": max(v) * 1e3 / g}
    for k, s in sims.items():
        res[k]["kernel"] = s.stats()["kernel"]
        res[k]["population"] = int(s.population())
    res["ltl R1 / rule@1"] = res["ltl@1 R1"]["us_per_gen"] / res["rule@1"]["us_per_gen"]
    if not a.skip_torch:
        res["torch R5 / ltl R5"] = res["torch R5"]["us_per_gen"] / res["ltl@1 R5"]["us_per_gen"]
        res["torch R7 / ltl R7"] = res["torch R7"]["us_per_gen"] / res["ltl@1 R7"]["us_per_gen"]
    print(json.dumps(res), flush=True)
    rows.append(res)
    del sims, variants

print()
print(f"{'N':>6} {'leg':<10} {'us/gen':>10} {'min':>10} {'max':>10}  kernel")
for res in rows:
    for k in ("ltl@1 R1", "rule@1", "ltl@1 R5", "ltl@1 R7", "torch R5", "torch R7"):
        if k in res:
            v = res[k]
            print(f"{res['N']:>6} {k:<10} {v['us_per_gen']:>10.2f} {v['min_us']:>10.2f} {v['max_us']:>10.2f}  {v.get('kernel', '')}")
    print(f"{res['N']:>6} ltl R1 / rule@1 = {res['ltl R1 / rule@1']:.2f}" +
          (f"   torch/ltl: R5 {res['torch R5 / ltl R5']:.1f}x, R7 {res['torch R7 / ltl R7']:.1f}x" if 'torch R5 / ltl R5' in res else ""))
