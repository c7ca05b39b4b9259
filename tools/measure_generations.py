"""Times the Generations kernel step_gen (docs/PERFORMANCE.md, "Generations rules") on one GPU, for each of --rules at
each of --sizes, from a board of random states:

  gen@Kmax  Simulation(rule=...) at the deepest pass of the rule's plane count: step(n), us per generation
  gen@1     the same at kernel_depth = halo_depth = 1
  rule@K    the two-state rule with the same B and S at the same K = Kmax (a pass moves 1 / (1 + M) of the bytes)
  torch     what a user would write today: a loop over a device uint8 tensor of states with a conv2d neighbour count of
            the live cells and where(); --torch-gens generations, us per generation
  counts    state_counts() (k_state_counts: only C counts leave the device) against board() plus np.bincount

Every figure is the median of --reps timed calls after one warm-up call, the legs of one rule and size interleaved
round by round in this one process: the three stepping legs and the torch loop in one set, the two census legs in a
second.  One JSON line per rule and size, then a table.

    python tools/measure_generations.py [--sizes 8192,32768] [--rules B2/S/C3,B2/S345/C4,B2/S345/C9] [--gens 240] [--reps 5]
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
ap.add_argument("--rules", default="B2/S/C3,B2/S345/C4,B2/S345/C9")
ap.add_argument("--gens", type=int, default=240, help="generations per timed step() call (a multiple of every Kmax)")
ap.add_argument("--torch-gens", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-torch", action="store_true")
ap.add_argument("--backend", default="hip")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gol_amd  # noqa: E402
from gol_amd.ops import parse_generations_rule  # noqa: E402


def clock(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def interleaved(variants, reps):
    """{name: (fn, sync)} -> {name: [ms]}: one warm-up round, then `reps` rounds, each timing every variant once."""
    out = {k: [] for k in variants}
    for r in range(reps + 1):
        for k, (fn, sync) in variants.items():
            ms = clock(fn, sync)
            if r:
                out[k].append(ms)
    return out


def summary(ms, gens):
    return {"us_per_gen": statistics.median(ms) * 1e3 / gens, "min_us": min(ms) * 1e3 / gens, "max_us": max(ms) * 1e3 / gens}


def torch_loop(states, birth, survive, C, gens):
    """`gens` generations of the rule on a device uint8 tensor of states, the way one writes it with torch."""
    import torch
    import torch.nn.functional as F

    ft = torch.float16 if states.is_cuda else torch.float32  # (counts up to 8 are exact in either)
    kernel = torch.ones((1, 1, 3, 3), dtype=ft, device=states.device)
    kernel[0, 0, 1, 1] = 0
    b_lut = torch.tensor([(birth >> c) & 1 for c in range(9)], dtype=torch.bool, device=states.device)
    s_lut = torch.tensor([(survive >> c) & 1 for c in range(9)], dtype=torch.bool, device=states.device)
    x = states
    for _ in range(gens):
        live = (x == 1).to(ft)[None, None]
        n = F.conv2d(F.pad(live, (1, 1, 1, 1), mode="circular"), kernel)[0, 0].to(torch.int64)
        born = (x == 0) & b_lut[n]
        stays = (x == 1) & s_lut[n]
        decay = torch.where(x + 1 < C, x + 1, torch.zeros_like(x))  # a dying cell, or a live one that starts to die
        x = torch.where(born | stays, torch.ones_like(x), torch.where(x == 0, x, decay))
    return x


def main():
    rows = []
    for N in (int(v) for v in a.sizes.split(",")):
        for rule in a.rules.split(","):
            birth, survive, C = parse_generations_rule(rule)
            kmax = gol_amd.native.max_generations_depth(C)
            two = rule.rsplit("/", 1)[0]
            n = a.gens - a.gens % kmax
            # half the cells dead, three in ten alive, the rest spread over the dying states (in bands of rows: bytes only)
            rng = np.random.default_rng(N + C)
            states = np.empty((N, N), np.uint8)
            lut = np.array([0] * 5 + [1] * 3 + [2] * 2, np.uint8)
            for r0 in range(0, N, 1024):
                band = lut[rng.integers(0, 10, size=(min(1024, N - r0), N), dtype=np.uint8)]
                dying = band == 2
                band[dying] += rng.integers(0, C - 2, size=int(dying.sum()), dtype=np.uint8)
                states[r0 : r0 + 1024] = band
            kw = dict(backend=a.backend)
            if a.backend == "hip":
                kw["device"] = 0
            sims = {
                f"gen@{kmax}": gol_amd.Simulation(N, rule=rule, halo_depth=kmax, kernel_depth=kmax, **kw).init(0),
                "gen@1": gol_amd.Simulation(N, rule=rule, halo_depth=1, kernel_depth=1, **kw).init(0),
                f"rule@{kmax}": gol_amd.Simulation(N, rule=two, kernel="rule", halo_depth=kmax, kernel_depth=kmax, **kw).init(0),
            }
            res = {"size": N, "rule": rule, "states": C, "gens": n, "reps": a.reps, "kernels": {}}
            for name, s in sims.items():
                s.set_board(states if s.states > 2 else (states == 1).astype(np.uint8))
                res["kernels"][name] = s.stats()["kernel"]
            variants = {name: ((lambda s=s: s.step(n)), s.synchronize) for name, s in sims.items()}
            gens_of = {name: n for name in sims}
            if not a.skip_torch and a.backend == "hip":
                import torch

                x = torch.from_numpy(states).to("cuda:0")
                variants["torch"] = ((lambda: torch_loop(x, birth, survive, C, a.torch_gens)), torch.cuda.synchronize)
                gens_of["torch"] = a.torch_gens
            for name, ms in interleaved(variants, a.reps).items():
                res[name] = summary(ms, gens_of[name])
            variants.pop("torch", None)
            x = None
            g = sims[f"gen@{kmax}"]
            got = {}

            def counts_new():
                got["new"] = g.state_counts()

            def counts_old():
                got["old"] = np.bincount(g.board().ravel(), minlength=C)

            for name, ms in interleaved({"state_counts": (counts_new, g.synchronize), "board+bincount": (counts_old, g.synchronize)},
                                        a.reps).items():
                res[name] = {"ms": statistics.median(ms)}
            assert got["new"].tolist() == got["old"].tolist()
            res["state_counts_values"] = got["new"].tolist()
            res["gen_over_rule"] = res[f"gen@{kmax}"]["us_per_gen"] / res[f"rule@{kmax}"]["us_per_gen"]
            res["gen1_over_genK"] = res["gen@1"]["us_per_gen"] / res[f"gen@{kmax}"]["us_per_gen"]
            print(json.dumps(res), flush=True)
            rows.append((N, rule, kmax, res))
            del sims, g
    print(f"{'size':>6} {'rule':<12} {'K':>2} {'gen@K':>9} {'gen@1':>9} {'rule@K':>9} {'torch':>10} {'gen/rule':>8} {'counts ms':>10} {'bincount ms':>11}")
    for N, rule, kmax, r in rows:
        t = r.get("torch", {}).get("us_per_gen", float("nan"))
        print(f"{N:>6} {rule:<12} {kmax:>2} {r[f'gen@{kmax}']['us_per_gen']:>9.2f} {r['gen@1']['us_per_gen']:>9.2f} "
              f"{r[f'rule@{kmax}']['us_per_gen']:>9.2f} {t:>10.1f} {r['gen_over_rule']:>8.2f} {r['state_counts']['ms']:>10.3f} "
              f"{r['board+bincount']['ms']:>11.1f}")


if __name__ == "__main__":
    main()
