"""Time `MicroCellPlan.secant` of a law with a history variable beside the same law with the history replaced by a constant, and
beside the host round trip it replaces -> profiles/secant_history_bench.json.

Workloads: the headline batch of 8,192 cells of 32² Poisson with the damage law c (1 - 0.5 (1 - exp(-kappa / 0.7))),
kappa = max(h, |e|), and 256 cells of 16³ elasticity with the shear modulus damaged the same way.  Per workload:
  (i)   `secant(history=)` with a fixed `max_iter` and `tol = 0` (every cell runs every round), divided by the rounds;
  (ii)  `secant()` of the same law with `h[0]` replaced by the constant 0.25: what a round costs without the read and the write of
        n_el doubles per cell beside the two coefficient streams;
  (iii) one round of the route a user had before -- `reconstruct(fields=True)`, the law and the update in NumPy, `solve(coef)`;
  (iv)  (i) and (ii) through `secant_device` with every array resident on the device, timed between synchronisations: a host call
        moves the history in and out once per call, whatever the rounds, and this pair shows a round without that.
Then `solve_nonlinear(method="newton")` to `tol = 1e-10` on a 16 x 16 macro mesh of 32² Poisson boxes (the 512 cells of
profiles/secant_tangent_bench.json) with the damage law and with its constant twin: what the host-held history costs per call.
Protocol of profiles/secant_bench.json throughout: host arrays in, after one warm-up of every route three rounds in which the routes
alternate; medians.

    python tools/bench_secant_history.py [--cells2d 8192] [--cells3d 256] [--iters 8] [--out profiles/secant_history_bench.json]
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

EQ = "sqrt(e[0]**2 + e[1]**2)"


def damage(kappa):
    return f"(1 - 0.5*(1 - exp(-{kappa}/0.7)))"


WITH, WITHOUT = damage(f"max(h[0], {EQ})"), damage(f"max(0.25, {EQ})")
UPDATE = [f"max(h[0], {EQ})"]
LAWS = {
    "poisson2d_32_damage": (2, 32, "poisson", SecantLaw(f"c[0]*{WITH}", history=UPDATE), SecantLaw(f"c[0]*{WITHOUT}")),
    "elasticity3d_16_damaged_shear": (3, 16, "elasticity", SecantLaw(lam="c[0]", mu=f"c[1]*{WITH}", history=UPDATE),
                                      SecantLaw(lam="c[0]", mu=f"c[1]*{WITHOUT}")),
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


def resident(p, nc, coef, xi, rows, h, law, constant, iters):
    """The two device calls on arrays that lie on the device, each timed to its synchronisation."""
    import torch

    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    src = CoefStream.sampled(coef).coef_source(upload)
    d_xi, d_rows, h_in = upload(xi), upload(rows), upload(h)
    state, A, h_out = (torch.empty(shape, dtype=torch.float64, device=dev) for shape in ((nc, 3), (nc, p.t, p.t), h.shape))

    def run(which, **kw):
        p.secant_device(nc, src, None, d_xi, which, d_rows, state.data_ptr(), A.data_ptr(), max_iter=iters, tol=0.0, **kw)
        torch.cuda.synchronize(dev)
        return keep  # the arrays live as long as the routes

    return {"history_resident": lambda: run(law, history_in_ptr=h_in, history_out_ptr=h_out.data_ptr()),
            "constant_resident": lambda: run(constant)}


def plan_level(dim, n, kind, nc, law, constant, iters, rounds, rng):
    p = MicroCellPlan(dim, n, kind)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    coef = np.exp(rng.uniform(-1.0, 1.0, (nc,) + el))
    xi = rng.standard_normal((nc, p.t))
    rows = np.zeros((nc, 3))
    h = np.full((nc, p.n_el, 1), 0.25)

    def host_round():
        r = p.reconstruct(coef, xi, fields=True)
        v = law.host_values(r.strain, r.flux, coef, rows, history=h)
        law.host_history(r.strain, r.flux, coef, rows, history=h)
        return p.solve(v.reshape(coef.shape))

    ms, every = timed({"history": lambda: p.secant(coef, xi, law, rows=rows, max_iter=iters, tol=0.0, history=h),
                       "constant": lambda: p.secant(coef, xi, constant, rows=rows, max_iter=iters, tol=0.0),
                       "host_round": host_round, **resident(p, nc, coef, xi, rows, h, law, constant, iters)}, rounds)
    for k in ("history", "constant", "history_resident", "constant_resident"):
        ms[k + "_per_round"] = ms[k] / iters
    ratios = {"history_round_over_constant_round": ms["history_per_round"] / ms["constant_per_round"],
              "host_round_over_history_round": ms["host_round"] / ms["history_per_round"],
              "resident_history_round_over_constant_round": ms["history_resident_per_round"] / ms["constant_resident_per_round"]}
    out = {"cells": nc, "n_el": p.n_el, "t": p.t, "iters": iters, "corrector_kernel": p.corrector_kernel, "ms": ms, "ratios": ratios,
           "all_ms": every}
    p.close()
    return out


def macro_level(nx, n, tol, rounds):
    solvers, routes = {}, {}
    for name, law in (("history", LAWS["poisson2d_32_damage"][3]), ("constant", LAWS["poisson2d_32_damage"][4])):
        A = hmm.TwoPhase(lambda y: (y[0] - 0.5) ** 2 + (y[1] - 0.5) ** 2 < 0.09, lambda x: 10.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
        h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: 40.0 + 0.0 * x[0], mesh.create_unit_square(n, n), 0.05)
        h.prepare(newton=True)

        def run(h=h, law=law):
            h._needs_reassembly = True
            if law.n_history:
                h.reset_history(np.full((h._local_cell_count(), h._cell_mesh.num_cells, 1), 0.25))
            h.solve_nonlinear(law, max_iter=100, tol=tol, micro_tol=1e-12, micro_iter=200, method="newton")

        solvers[name], routes[name] = h, run
    ms, every = timed(routes, rounds)
    out = {m: {"macro_steps": len(h.nonlinear_history), "micro_rounds": int(h.secant.rounds.sum()), "wall_ms": ms[m], "all_ms": every[m],
               "last_change": h.nonlinear_history[-1]} for m, h in solvers.items()}
    out["history_over_constant"] = ms["history"] / ms["constant"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells2d", type=int, default=8192)
    ap.add_argument("--cells3d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--macro", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "secant_history_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    result = {"protocol": f"host arrays in; one warm-up, then {a.rounds} rounds with the routes alternating; medians, milliseconds; "
                          f"{a.iters} rounds at tol = 0, the whole call and per round", "workloads": {}}
    cells = {"poisson2d_32_damage": a.cells2d, "elasticity3d_16_damaged_shear": a.cells3d}
    for name, (dim, n, kind, law, constant) in LAWS.items():
        w = result["workloads"][name] = plan_level(dim, n, kind, cells[name], law, constant, a.iters, a.rounds, rng)
        print(name, {k: round(v, 2) for k, v in w["ms"].items()}, {k: round(v, 3) for k, v in w["ratios"].items()}, flush=True)
    result["solve_nonlinear"] = dict(macro_cells=2 * a.macro * a.macro, n=32, tol=1e-10, method="newton", **macro_level(a.macro, 32, 1e-10, a.rounds))
    print("solve_nonlinear", result["solve_nonlinear"], flush=True)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
