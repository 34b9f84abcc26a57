"""Time the criterion tail of the secant iteration against the detour it replaces -> profiles/secant_state_bench.json.

Workloads: the headline batch of 8,192 cells of 32² Poisson with the softening law c (0.5 + 0.5 / (1 + |e|^2)), and 256 cells of 16³
elasticity with the shear modulus softened the same way.  The criterion is the flux norm over the base coefficient,
sqrt(sum s_k^2) / b[0] (routes iii and iv, which have no base, divide by c[0]: the same work).  Per workload, a fixed `max_iter` at
`tol = 0` (every cell runs every round):
  (i)   `secant_device` without a tail;
  (ii)  `secant_device` with the criterion tail: four numbers per cell are written beside the iteration's outputs;
  (iii) the route of the parent commit with device pointers: `secant_device(coef_ptr=...)`, then `criterion_device` on that stream --
        the stream stays on the device, every cell is eliminated once more;
  (iv)  route (iii) through host arrays, `secant(return_coef=True)` then `criterion(coef_out)`, as the solver classes would have had to
        do it: n_el n_comp doubles per cell to the host and back.
(i) - (iii) with every array resident on the device, timed between synchronisations.  Protocol of profiles/secant_load_bench.json:
after one warm-up of every route three rounds in which the routes alternate; medians.

    python tools/bench_secant_state.py [--cells2d 8192] [--cells3d 256] [--iters 8] [--out profiles/secant_state_bench.json]
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
from hommx_amd.batch import CoefStream  # noqa: E402
from hommx_amd.expr import Criterion, SecantLaw  # noqa: E402

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


def workload(dim, n, kind, nc, law, iters, rounds, rng):
    import torch

    p = MicroCellPlan(dim, n, kind)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    norm = " + ".join(f"s[{k}]**2" for k in range(p.t))
    state_crit, linear_crit = Criterion(f"sqrt({norm})/b[0]"), Criterion(f"sqrt({norm})/c[0]")
    coef, xi, rows = np.exp(rng.uniform(-1.0, 1.0, (nc,) + el)), rng.standard_normal((nc, p.t)), np.zeros((nc, 3))
    src = CoefStream.sampled(coef).coef_source(upload)
    d_xi, d_rows = upload(xi), upload(rows)
    state, A, crit = (torch.empty(shape, dtype=torch.float64, device=dev) for shape in ((nc, 3), (nc, p.t, p.t), (nc, 4)))
    out_coef = torch.empty((nc,) + el, dtype=torch.float64, device=dev)
    out_src = CoefStream.sampled(coef).coef_source(lambda a: out_coef.data_ptr())

    def secant(**kw):
        p.secant_device(nc, src, None, d_xi, law, d_rows, state.data_ptr(), A.data_ptr(), max_iter=iters, tol=0.0, **kw)

    def plain():
        secant()
        torch.cuda.synchronize(dev)

    def tail():
        secant(criterion=state_crit, crit_rows_ptr=d_rows, crit_ptr=crit.data_ptr())
        torch.cuda.synchronize(dev)

    def detour_device():
        secant(coef_ptr=out_coef.data_ptr())
        p.criterion_device(nc, out_src, None, d_xi, linear_crit, d_rows, crit.data_ptr())
        torch.cuda.synchronize(dev)

    def detour_host():
        r = p.secant(coef, xi, law, rows=rows, max_iter=iters, tol=0.0, return_coef=True)
        p.criterion(r.coef, xi, linear_crit, rows=rows)

    ms, every = timed({"secant": plain, "secant_with_tail": tail, "detour_device": detour_device, "detour_host": detour_host}, rounds)
    ratios = {"tail_ms": ms["secant_with_tail"] - ms["secant"], "round_ms": ms["secant"] / iters,
              "tail_over_round": (ms["secant_with_tail"] - ms["secant"]) / (ms["secant"] / iters),
              "detour_device_over_tail": ms["detour_device"] / ms["secant_with_tail"],
              "detour_host_over_tail": ms["detour_host"] / ms["secant_with_tail"]}
    out = {"cells": nc, "n_el": p.n_el, "t": p.t, "iters": iters, "corrector_kernel": p.corrector_kernel,
           "stream_megabytes": 8e-6 * nc * p.n_el * p.n_comp, "ms": ms, "ratios": ratios, "all_ms": every}
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells2d", type=int, default=8192)
    ap.add_argument("--cells3d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "secant_state_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    result = {"protocol": f"routes (i) - (iii) with every array resident on the device, route (iv) through host arrays; one warm-up, then "
                          f"{a.rounds} rounds with the routes alternating; medians, milliseconds; {a.iters} rounds at tol = 0, the whole call",
              "workloads": {}}
    cells = {"poisson2d_32": a.cells2d, "elasticity3d_16_softened_shear": a.cells3d}
    for name, (dim, n, kind, law) in LAWS.items():
        w = result["workloads"][name] = workload(dim, n, kind, cells[name], law, a.iters, a.rounds, rng)
        print(name, {k: round(v, 2) for k, v in w["ms"].items()}, {k: round(v, 3) for k, v in w["ratios"].items()}, flush=True)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
