"""Time `MicroCellPlan.secant_tangent` beside `secant` with the same rounds, and `solve_nonlinear` with `method="newton"` beside
`method="secant"` -> profiles/secant_tangent_bench.json.

Workloads: the headline batch of 8,192 cells of 32² Poisson with the potential law c (0.5 + 0.5 / (1 + |e|²)), and 256 cells of 16³
elasticity with mu = c1 (0.5 + 0.5 / (1 + eps:eps)).  Per workload:
  (i)   `secant()` and `secant_tangent()` with a fixed `max_iter` and `tol = 0` (every cell runs every round): the difference is the
        tangent pass plus one elimination of the tangent kind;
  (ii)  that elimination alone: `tangent_plan.solve_device()` of a tangent stream of the same batch that already lies on the device,
        timed between synchronisations -- what the chunk runs, without a transfer.  (i) - (ii) is then the tangent pass with the
        transfer of D and the asymmetry.
Then `solve_nonlinear` to `tol = 1e-10` on a 16 x 16 macro mesh of 32² Poisson boxes, both methods, each on a solver of its own whose
plans (the sibling included) exist before the clock starts: macro steps, total micro rounds, wall time.
Protocol of profiles/secant_bench.json throughout: after one warm-up of every route, three rounds in which the routes alternate; medians.

    python tools/bench_secant_tangent.py [--cells2d 8192] [--cells3d 256] [--iters 8] [--out profiles/secant_tangent_bench.json]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hommx_amd import MicroCellPlan, hmm, mesh  # noqa: E402
from hommx_amd.expr import SecantLaw  # noqa: E402

LAW2D = SecantLaw("c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))")
LAW3D = SecantLaw(lam="c[0]", mu="c[1]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2 + e[2]**2 + 0.5*e[3]**2 + 0.5*e[4]**2 + 0.5*e[5]**2))")


def timed(routes, rounds):
    times = {k: [] for k in routes}
    for f in routes.values():
        f()
    for _ in range(rounds):
        for k, f in routes.items():
            t0 = time.perf_counter()
            f()
            times[k].append(1e3 * (time.perf_counter() - t0))
    return {k: statistics.median(v) for k, v in times.items()}, times


def plan_level(dim, n, kind, nc, law, iters, rounds, rng):
    import torch

    p = MicroCellPlan(dim, n, kind)
    q = MicroCellPlan(dim, n, p.tangent_kind)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    coef = np.exp(rng.uniform(-1.0, 1.0, (nc,) + el))
    xi = rng.standard_normal((nc, p.t))
    rows = np.zeros((nc, 3))
    dev = torch.device("cuda", q.device)
    stream = torch.from_numpy(p.secant_tangent(coef, xi, law, q, rows=rows, max_iter=iters, tol=0.0, return_tangent_coef=True).tangent_coef).to(dev)
    D, info = torch.empty((nc, p.t, p.t), dtype=torch.float64, device=dev), torch.empty(nc, dtype=torch.int32, device=dev)

    def elimination():
        torch.cuda.synchronize(dev)
        q.solve_device(nc, stream.data_ptr(), None, D.data_ptr(), info.data_ptr(), None)
        torch.cuda.synchronize(dev)

    ms, every = timed({
        "secant": lambda: p.secant(coef, xi, law, rows=rows, max_iter=iters, tol=0.0),
        "secant_tangent": lambda: p.secant_tangent(coef, xi, law, q, rows=rows, max_iter=iters, tol=0.0),
        "tangent_elimination": elimination,
    }, rounds)
    ms["tangent_extra"] = ms["secant_tangent"] - ms["secant"]
    ms["tangent_pass"] = ms["tangent_extra"] - ms["tangent_elimination"]
    ratios = {"tangent_extra_over_secant_round": ms["tangent_extra"] / (ms["secant"] / iters)}
    out = {"cells": nc, "n_el": p.n_el, "t": p.t, "iters": iters, "corrector_kernel": p.corrector_kernel, "tangent_kernel": q.kernel, "ms": ms,
           "ratios": ratios, "all_ms": every}
    p.close()
    q.close()
    return out


def macro_level(nx, n, tol, rounds):
    solvers, counts, routes = {}, {}, {}
    for method in ("secant", "newton"):
        A = hmm.TwoPhase(lambda y: (y[0] - 0.5) ** 2 + (y[1] - 0.5) ** 2 < 0.09, lambda x: 10.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
        h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: 40.0 + 0.0 * x[0], mesh.create_unit_square(n, n), 0.05)
        h.prepare(newton=method == "newton")
        name = "secant_tangent" if method == "newton" else "secant"
        inner = getattr(h._plan, name)

        def counted(*a, _inner=inner, _method=method, **kw):
            r = _inner(*a, **kw)
            counts[_method].append(int(r.rounds.sum()))
            return r

        setattr(h._plan, name, counted)

        def run(h=h, method=method):
            counts[method] = []
            h._needs_reassembly = True
            h.solve_nonlinear(LAW2D, max_iter=100, tol=tol, micro_tol=1e-12, micro_iter=200, method=method)

        solvers[method], routes[method] = h, run
    ms, every = timed(routes, rounds)
    return {m: {"macro_steps": len(h.nonlinear_history), "micro_rounds": int(sum(counts[m])), "wall_ms": ms[m], "all_ms": every[m],
                "last_change": h.nonlinear_history[-1]} for m, h in solvers.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells2d", type=int, default=8192)
    ap.add_argument("--cells3d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--macro", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "secant_tangent_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    result = {"protocol": f"one warm-up, then {a.rounds} rounds with the routes alternating; medians, milliseconds; {a.iters} rounds at "
                          "tol = 0 in secant and secant_tangent alike", "workloads": {}}
    for name, (dim, n, kind, nc, law) in {"poisson2d_32": (2, 32, "poisson", a.cells2d, LAW2D),
                                          "elasticity3d_16": (3, 16, "elasticity", a.cells3d, LAW3D)}.items():
        result["workloads"][name] = plan_level(dim, n, kind, nc, law, a.iters, a.rounds, rng)
        print(name, {k: round(v, 2) for k, v in result["workloads"][name]["ms"].items()}, flush=True)
    result["solve_nonlinear"] = dict(macro_cells=2 * a.macro * a.macro, n=32, tol=1e-10, **macro_level(a.macro, 32, 1e-10, a.rounds))
    print("solve_nonlinear", result["solve_nonlinear"], flush=True)
    if a.out != "/dev/null":
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
