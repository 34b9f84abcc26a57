"""Time `MicroCellPlan.secant` per round beside `reconstruct` and the host round trip it replaces -> profiles/secant_bench.json.

Workloads: the headline batch of 8,192 cells of 32² Poisson with the softening law c (0.5 + 0.5 / (1 + |e|²)), and 256 cells of 16³
elasticity with the shear modulus softened the same way.  Per workload:
  (i)   `secant()` with a fixed `max_iter` and `tol = 0` (every cell runs every round), divided by the rounds;
  (ii)  `reconstruct()` of the same batch (statistics alone): one elimination plus one element walk, what a round is made of;
  (iii) one round of the route a user had before -- `reconstruct(fields=True)`, `SecantLaw.host_values`, `solve(coef)`.
Protocol of profiles/criterion_bench.json: after one warm-up of every route, three rounds in which the routes alternate; medians.

    python tools/bench_secant.py [--cells2d 8192] [--cells3d 256] [--iters 8] [--out profiles/secant_bench.json]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hommx_amd import MicroCellPlan  # noqa: E402
from hommx_amd.expr import SecantLaw  # noqa: E402

SOFT = "(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"


def workload(dim, n, kind, nc, law, iters, rng):
    p = MicroCellPlan(dim, n, kind)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    coef = np.exp(rng.uniform(-1.0, 1.0, (nc,) + el))
    xi = rng.standard_normal((nc, p.t))
    rows = np.zeros((nc, 3))

    def host_round():
        r = p.reconstruct(coef, xi, fields=True)
        v = law.host_values(r.strain, r.flux, coef, rows)
        return p.solve(v.reshape(coef.shape))

    routes = {
        "secant": lambda: p.secant(coef, xi, law, rows=rows, max_iter=iters, tol=0.0),
        "reconstruct": lambda: p.reconstruct(coef, xi),
        "host_round": host_round,
    }
    return p, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells2d", type=int, default=8192)
    ap.add_argument("--cells3d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "secant_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    result = {"protocol": f"one warm-up, then {a.rounds} rounds with the routes alternating; medians, milliseconds; secant: {a.iters} rounds "
                          "at tol = 0, the whole call and per round", "workloads": {}}
    for name, (dim, n, kind, nc, law) in {
        "poisson2d_32_softening": (2, 32, "poisson", a.cells2d, SecantLaw(f"c[0]*{SOFT}")),
        "elasticity3d_16_softening_shear": (3, 16, "elasticity", a.cells3d, SecantLaw(lam="c[0]", mu=f"c[1]*{SOFT}")),
    }.items():
        p, routes = workload(dim, n, kind, nc, law, a.iters, rng)
        times = {k: [] for k in routes}
        for k, f in routes.items():
            f()
        for _ in range(a.rounds):
            for k, f in routes.items():
                t0 = time.perf_counter()
                f()
                times[k].append(1e3 * (time.perf_counter() - t0))
        ms = {k: statistics.median(v) for k, v in times.items()}
        ms["secant_per_round"] = ms["secant"] / a.iters
        ratios = {"secant_round_over_reconstruct": ms["secant_per_round"] / ms["reconstruct"],
                  "host_round_over_secant_round": ms["host_round"] / ms["secant_per_round"]}
        result["workloads"][name] = {"cells": nc, "n_el": p.n_el, "t": p.t, "iters": a.iters, "corrector_kernel": p.corrector_kernel, "ms": ms,
                                     "ratios": ratios, "all_ms": times}
        print(name, {k: round(v, 2) for k, v in ms.items()}, {k: round(v, 2) for k, v in ratios.items()}, flush=True)
        p.close()
    if a.out != "/dev/null":
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
