"""Throughput of the mesh route (csrc/mesh_front.hip) at 8,192 macro cells: solves/s, front width, flops model, TF/s.

    python tools/bench_mesh.py [--cells 8192] [--reps 5] [--out profiles/mesh_bench.json]

Device pointers (torch tensors), coefficient already resident: the kernel rate, as bench.py measures the structured routes.  The
last case runs create_unit_square(32, 32) through the mesh route next to the fused route's rate on the same coefficients."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from hommx_amd import MicroCellPlan, mesh as Mm, workloads as W  # noqa: E402


def rate(plan, coef, reps):
    nc = coef.shape[0]
    out = torch.empty((nc, plan.t, plan.t), dtype=torch.float64, device="cuda")
    info = torch.empty(nc, dtype=torch.int32, device="cuda")
    plan.solve_device(nc, coef.data_ptr(), None, out.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        plan.solve_device(nc, coef.data_ptr(), None, out.data_ptr(), info.data_ptr())
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    assert int((info != 0).sum()) == 0
    return nc / best, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    cases = [
        ("jittered 32x32 2D Poisson", W.jittered_unit_square(32, 32), "poisson"),
        ("jittered 40x40 2D elasticity (front near the limit)", W.jittered_unit_square(40, 40), "elasticity"),
        ("jittered 6x6x6 3D Poisson", W.jittered_unit_cube(6, 6, 6), "poisson"),
        ("create_unit_square(32, 32) through the mesh route", Mm.create_unit_square(32, 32), "poisson"),
    ]
    rows = []
    for name, msh, kind in cases:
        p = MicroCellPlan.from_mesh(msh, kind)
        shape = (a.cells, p.n_el) + ((p.n_comp,) if p.n_comp > 1 else ())
        host = rng.uniform(0.5, 2.0, shape)
        if kind == "elasticity":
            host[..., 0] *= 0.5
        coef = torch.from_numpy(host).cuda()
        sps, sec = rate(p, coef, a.reps)
        row = {"case": name, "kind": kind, "cells": a.cells, "n_nodes": p.n_nodes, "n_el": p.n_el, "front_width": p.front_width,
               "flops_per_solve": p.flops_per_solve, "seconds": sec, "solves_per_s": sps, "tflops": sps * p.flops_per_solve / 1e12,
               "route": p.route_detail}
        if msh.shape == (32, 32):
            q = MicroCellPlan(2, 32, "poisson")
            fsps, _ = rate(q, coef, a.reps)
            row["fused_route_solves_per_s"] = fsps
        rows.append(row)
        print(json.dumps(row), flush=True)
        del coef
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
