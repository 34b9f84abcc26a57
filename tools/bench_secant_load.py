"""Time a round of the secant iteration beside a load against a round without one, and `solve_nonlinear(load=True)` against
`load=False` -> profiles/secant_load_bench.json.

Workloads: the headline batch of 8,192 cells of 32² Poisson with the softening law c (0.5 + 0.5 / (1 + |e|^2)) -- the load solve is
the substitution on the fused factor records --, and 256 cells of 16³ elasticity with the shear modulus softened the same way -- the
load solve is a blocked pass.  Per workload, through `secant_device` with every array resident on the device, timed between
synchronisations, a fixed `max_iter` at `tol = 0` (every cell runs every round), divided by the rounds:
  (i)   no load;
  (ii)  a per-cell polarisation: per round one load solve more, chi_P and P read by the round kernel;
  (iii) a per-cell eigenstrain: the eigenstress of the round as well.
Then `solve_nonlinear` to `tol = 1e-10` on a 16 x 16 macro mesh of 32² Poisson boxes (the 512 cells of
profiles/secant_tangent_bench.json), both methods, with a thermal eigenstrain (`load=True`) and without one.
Protocol of profiles/secant_bench.json: after one warm-up of every route three rounds in which the routes alternate; medians.

    python tools/bench_secant_load.py [--cells2d 8192] [--cells3d 256] [--iters 8] [--out profiles/secant_load_bench.json]
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
from hommx_amd.batch import CoefStream  # noqa: E402
from hommx_amd.expr import SecantLaw  # noqa: E402

SOFT = "(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"
LAWS = {
    "poisson2d_32": (2, 32, "poisson", SecantLaw(f"c[0]*{SOFT}")),
    "elasticity3d_16_softened_shear": (3, 16, "elasticity", SecantLaw(lam="c[0]", mu=f"c[1]*{SOFT}")),
}


def timed(routes, rounds):
    for f in routes.values():
        f()
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, f in routes.items():
            t0 = time.perf_counter()
            f()
            times[k].append(1e3 * (time.perf_counter() - t0))
    return {k: statistics.median(v) for k, v in times.items()}, times


def plan_level(dim, n, kind, nc, law, iters, rounds, rng):
    import torch

    p = MicroCellPlan(dim, n, kind)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    src = CoefStream.sampled(np.exp(rng.uniform(-1.0, 1.0, (nc,) + el))).coef_source(upload)
    d_xi, d_rows = upload(rng.standard_normal((nc, p.t))), upload(np.zeros((nc, 3)))
    d_load = upload(0.3 * rng.standard_normal((nc, p.n_el, p.t)))
    state, A = (torch.empty(shape, dtype=torch.float64, device=dev) for shape in ((nc, 3), (nc, p.t, p.t)))

    def run(**kw):
        p.secant_device(nc, src, None, d_xi, law, d_rows, state.data_ptr(), A.data_ptr(), max_iter=iters, tol=0.0, **kw)
        torch.cuda.synchronize(dev)
        return keep  # the arrays live as long as the routes

    ms, every = timed({"no_load": run, "polarisation": lambda: run(P_ptr=d_load), "eigenstrain": lambda: run(P_ptr=d_load, eigenstrain=True)},
                      rounds)
    for k in ("no_load", "polarisation", "eigenstrain"):
        ms[k + "_per_round"] = ms[k] / iters
    ratios = {"polarisation_round_over_round": ms["polarisation_per_round"] / ms["no_load_per_round"],
              "eigenstrain_round_over_round": ms["eigenstrain_per_round"] / ms["no_load_per_round"]}
    out = {"cells": nc, "n_el": p.n_el, "t": p.t, "iters": iters, "corrector_kernel": p.corrector_kernel, "load_kernel": p.load_kernel, "ms": ms,
           "ratios": ratios, "all_ms": every}
    p.close()
    return out


def macro_level(nx, n, tol, rounds):
    solvers, routes = {}, {}
    law = LAWS["poisson2d_32"][3]
    for load in (False, True):
        for method in ("secant", "newton"):
            A = hmm.TwoPhase(lambda y: (y[0] - 0.5) ** 2 + (y[1] - 0.5) ** 2 < 0.09, lambda x: 10.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
            h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: 40.0 + 0.0 * x[0], mesh.create_unit_square(n, n), 0.05)
            if load:  # a thermal strain alpha(y) dT(x) I, the inclusion expanding three times as much as the matrix
                h.set_eigenstrain(hmm.Expression(["where((y[0] - 0.5)**2 + (y[1] - 0.5)**2 < 0.09, 0.03, 0.01)*f[0]"] * 2, fields=("dT",)))
                h.set_polarisation_fields(10.0 + 20.0 * h._msh.cell_midpoints()[:, 0])
            h.prepare(newton=method == "newton")

            def run(h=h, method=method, load=load):
                h._needs_reassembly = True
                h.solve_nonlinear(law, max_iter=100, tol=tol, micro_tol=1e-12, micro_iter=200, method=method, load=load)

            name = f"{method}_{'load' if load else 'no_load'}"
            solvers[name], routes[name] = h, run
    ms, every = timed(routes, rounds)
    out = {m: {"macro_steps": len(h.nonlinear_history), "micro_rounds": int(h.secant.rounds.sum()), "wall_ms": ms[m], "all_ms": every[m],
               "last_change": h.nonlinear_history[-1]} for m, h in solvers.items()}
    for method in ("secant", "newton"):
        a, b = out[f"{method}_load"], out[f"{method}_no_load"]
        out[f"{method}_load_over_no_load_per_micro_round"] = (a["wall_ms"] / a["micro_rounds"]) / (b["wall_ms"] / b["micro_rounds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells2d", type=int, default=8192)
    ap.add_argument("--cells3d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--macro", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "secant_load_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    result = {"protocol": f"every array resident on the device; one warm-up, then {a.rounds} rounds with the routes alternating; medians, "
                          f"milliseconds; {a.iters} rounds at tol = 0, the whole call and per round", "workloads": {}}
    cells = {"poisson2d_32": a.cells2d, "elasticity3d_16_softened_shear": a.cells3d}
    for name, (dim, n, kind, law) in LAWS.items():
        w = result["workloads"][name] = plan_level(dim, n, kind, cells[name], law, a.iters, a.rounds, rng)
        print(name, {k: round(v, 2) for k, v in w["ms"].items()}, {k: round(v, 3) for k, v in w["ratios"].items()}, flush=True)
    result["solve_nonlinear"] = dict(macro_cells=2 * a.macro * a.macro, n=32, tol=1e-10, **macro_level(a.macro, 32, 1e-10, a.rounds))
    print("solve_nonlinear", result["solve_nonlinear"], flush=True)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
