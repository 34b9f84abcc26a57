"""Throughput of the tree route of the mesh family (csrc/mesh_tree.hip on the multifrontal engine): solves/s, flops per solve, TF/s by the
route's model, fronts, groups and arena per cell.

    python tools/bench_mesh_tree.py [--scale 1.0] [--reps 3] [--out profiles/mesh_tree_bench.json]

Device pointers (torch tensors), coefficient already resident, workspace reserved ahead: the kernel rate, as bench.py measures the
structured routes.  The last case runs create_unit_cube(16, 16, 16) through the tree route next to the structured multifrontal route on
the same coefficients.  --scale multiplies every cell count (quick runs)."""

from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from hommx_amd import MicroCellPlan, mesh as Mm, workloads as W  # noqa: E402
from hommx_amd.batch import mesh_analyze_tree  # noqa: E402


def rate(plan, coef, reps):
    nc = coef.shape[0]
    plan.reserve(nc)
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
    return nc / best, best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    cases = [
        ("jittered 8x8x8 3D elasticity", W.jittered_unit_cube(8, 8, 8), "elasticity", 4096),
        ("jittered 12x12x12 3D elasticity", W.jittered_unit_cube(12, 12, 12), "elasticity", 1024),
        ("jittered 16x16x16 3D elasticity", W.jittered_unit_cube(16, 16, 16), "elasticity", 1024),
        ("jittered 12x12x12 3D Poisson", W.jittered_unit_cube(12, 12, 12), "poisson", 4096),
        ("jittered 128x128 2D Poisson", W.jittered_unit_square(128, 128), "poisson", 8192),
        ("create_unit_cube(16, 16, 16) through the tree route", Mm.create_unit_cube(16, 16, 16), "elasticity", 1024),
    ]
    rows = []
    for name, msh, kind, cells in cases:
        cells = max(1, int(cells * a.scale))
        p = MicroCellPlan.from_mesh(msh, kind, route="tree")
        tree = mesh_analyze_tree(msh, kind)
        shape = (cells, p.n_el) + ((p.n_comp,) if p.n_comp > 1 else ())
        host = rng.uniform(0.5, 2.0, shape)
        if kind == "elasticity":
            host[..., 0] *= 0.5
        coef = torch.from_numpy(host).cuda()
        sps, sec, out = rate(p, coef, a.reps)
        arena = re.search(r"arena ([0-9.]+) MB per cell", p.route_detail)
        row = {"case": name, "kind": kind, "cells": cells, "n_nodes": p.n_nodes, "n_el": p.n_el, "kernel": p.kernel,
               "flops_per_solve": p.flops_per_solve, "seconds": sec, "solves_per_s": sps, "tflops": sps * p.flops_per_solve / 1e12,
               "n_fronts": tree["n_fronts"], "n_groups": tree["n_groups"], "max_front": tree["max_front"],
               "arena_mb_per_cell": float(arena.group(1)) if arena else None, "route": p.route_detail}
        if msh.shape == (16, 16, 16):
            q = MicroCellPlan(3, 16, kind)
            qsps, _, qout = rate(q, coef, a.reps)
            row.update({"structured_kernel": q.kernel, "structured_solves_per_s": qsps, "structured_flops_per_solve": q.flops_per_solve,
                        "structured_tflops": qsps * q.flops_per_solve / 1e12, "tree_over_structured_time": qsps / sps,
                        "max_rel_diff_vs_structured": float((out - qout).abs().max() / qout.abs().max())})
            del q
        rows.append(row)
        print(json.dumps(row), flush=True)
        del coef, out, p
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
