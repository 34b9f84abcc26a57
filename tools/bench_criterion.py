"""Time `MicroCellPlan.criterion` beside `reconstruct` and the host round trip it replaces -> profiles/criterion_bench.json.

Workloads: the headline batch of 8,192 cells of 32² Poisson with `Criterion.flux_norm`, and 256 cells of 16³ elasticity with
`Criterion.von_mises`.  Per workload, with and without one per-cell load: `criterion()`; `reconstruct()` (statistics alone); the route a
criterion took before -- `reconstruct(fields=True)` (+ `loads(fields=True)`) followed by `Criterion.host_values`.  Protocol of
profiles/derived_driver_ab.json: after one warm-up of every route, three rounds in which the routes alternate; the median of each.

    python tools/bench_criterion.py [--cells2d 8192] [--cells3d 256] [--out profiles/criterion_bench.json]

The kernel time of k_criterion beside k_recon comes from a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_criterion.py --rounds 1 --out /dev/null
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
from hommx_amd.expr import Criterion  # noqa: E402


def workload(dim, n, kind, nc, crit, rng):
    p = MicroCellPlan(dim, n, kind)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    coef = np.exp(rng.uniform(-1.0, 1.0, (nc,) + el))
    xi = rng.standard_normal((nc, p.t))
    P = rng.standard_normal((nc, p.n_el, p.t))
    rows = np.zeros((nc, 3))

    def host_route(load):
        r = p.reconstruct(coef, xi, fields=True)
        e, s = r.strain, r.flux
        if load:
            lr = p.loads(coef, P[:, None], fields=True)
            e, s = e + lr.strain[:, 0], s + lr.flux[:, 0]
        return crit.host_values(e, s, coef, rows).max(axis=1)

    routes = {
        "criterion": lambda: p.criterion(coef, xi, crit, rows=rows),
        "criterion_with_load": lambda: p.criterion(coef, xi, crit, rows=rows, P=P),
        "reconstruct": lambda: p.reconstruct(coef, xi),
        "host_route": lambda: host_route(False),
        "host_route_with_load": lambda: host_route(True),
    }
    return p, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells2d", type=int, default=8192)
    ap.add_argument("--cells3d", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "criterion_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    result = {"protocol": f"one warm-up, then {a.rounds} rounds with the routes alternating; medians, milliseconds", "workloads": {}}
    for name, (dim, n, kind, nc, crit) in {
        "poisson2d_32_flux_norm": (2, 32, "poisson", a.cells2d, Criterion.flux_norm("poisson", 2)),
        "elasticity3d_16_von_mises": (3, 16, "elasticity", a.cells3d, Criterion.von_mises(3, strength="where(c[1] > 1, 4, 2)")),
    }.items():
        p, routes = workload(dim, n, kind, nc, crit, rng)
        times = {k: [] for k in routes}
        for k, f in routes.items():
            f()
        for _ in range(a.rounds):
            for k, f in routes.items():
                t0 = time.perf_counter()
                f()
                times[k].append(1e3 * (time.perf_counter() - t0))
        result["workloads"][name] = {"cells": nc, "n_el": p.n_el, "t": p.t, "corrector_kernel": p.corrector_kernel, "load_kernel": p.load_kernel,
                                     "ms": {k: statistics.median(v) for k, v in times.items()}, "all_ms": times}
        print(name, {k: round(statistics.median(v), 2) for k, v in times.items()}, flush=True)
        p.close()
    if a.out != "/dev/null":
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
