"""Cost of the load solve of the frontal mesh route (k_mesh_front_rhs) against the tree route of the same mesh -- until
HOMMX_MESH_FLAG_LOADS the only way to a load response on an unstructured micro mesh -- at 8,192 macro cells of the jittered 32 x 32 2D
Poisson mesh and of the jittered 6^3 3D Poisson mesh of profiles/mesh_bench.json.

    python tools/bench_mesh_loads.py [--cells 8192] [--reps 7] [--out profiles/mesh_front_loads_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_mesh_loads.py --case 2D --profile-leg response --reps 3
    python tools/bench_mesh_loads.py --case 2D --merge-kernel-stats response DIR/.../run_kernel_stats.csv --reps 3

Per case and plan -- from_mesh(route="front", load_solve=True) and from_mesh(route="tree") --, device entries, everything resident:
    response   hommx_loads_source_device with one load shared by all cells; energy and statistics, no fields
    second     hommx_second_sensitivity_source_device with two shared directions (t loads per direction and cell)
    canonical  hommx_sensitivity_source_device with one direction: the canonical corrector pass of the same chunks and one contraction
Median wall time of --reps calls after one warm-up call, the two plans alternating call by call.  --profile-leg runs one entry of the
frontal plan alone, for a kernel trace; --merge-kernel-stats adds the kernel times of that trace per API call: the model is the
canonical pass (k_mesh_front with the arena, k_mesh_backsub) plus about twice k_mesh_backsub per load block."""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"2D": ("jittered 32x32 2D Poisson", lambda W: W.jittered_unit_square(32, 32)),
         "3D": ("jittered 6x6x6 3D Poisson", lambda W: W.jittered_unit_cube(6, 6, 6))}
KERNELS = ("k_mesh_front_rhs", "k_mesh_front", "k_mesh_backsub", "k_polar", "k_load_stats", "k_sens2_loads", "k_sens2")


def entries(p, nc, rng):
    """{name: call} of the three device entries on plan `p`, and the info tensor they write."""
    import torch

    dev = torch.device("cuda", p.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    t = p.t
    coef, P, dirs = up(rng.uniform(0.5, 2.0, (nc, p.n_el))), up(rng.standard_normal((1, p.n_el, t))), up(rng.standard_normal((2, p.n_el)))
    P_eff, energy, stats, A, d2A, dA = new(nc, 1, t), new(nc, 1, 1), new(nc, 1, t + 2), new(nc, t, t), new(nc, 2, 2, t, t), new(nc, 1, t, t)
    info = torch.empty(nc, dtype=torch.int32, device=dev)
    from hommx_amd import _lib

    src = _lib.CoefSource()
    src.form, src.coef = _lib.COEF_SAMPLED, coef.data_ptr()
    s = torch.cuda.current_stream(dev).cuda_stream
    keep = (coef, P, dirs, P_eff, energy, stats, A, d2A, dA)
    return {
        "response": lambda: p.loads_device(nc, src, None, 1, P.data_ptr(), P_eff.data_ptr(), False, A.data_ptr(), info.data_ptr(), energy.data_ptr(),
                                           stats.data_ptr(), stream=s),
        "second": lambda: p.second_sensitivities_device(nc, src, None, 2, dirs.data_ptr(), d2A.data_ptr(), False, None, A.data_ptr(), info.data_ptr(),
                                                        stream=s),
        "canonical": lambda: p.sensitivities_device(nc, src, None, 1, dirs.data_ptr(), False, dA.data_ptr(), A_ptr=A.data_ptr(),
                                                    info_ptr=info.data_ptr(), stream=s),
    }, info, keep


def plans(msh):
    from hommx_amd import MicroCellPlan

    front, tree = MicroCellPlan.from_mesh(msh, "poisson", route="front", load_solve=True), MicroCellPlan.from_mesh(msh, "poisson", route="tree")
    assert front.load_kernel == "mesh_front_subst" and tree.load_kernel == "mesh_multifrontal", (front.load_kernel, tree.load_kernel)
    return {"front": front, "tree": tree}


def measure(nc, reps, only):
    import torch

    from hommx_amd import workloads as W

    out = []
    for key, (name, make) in CASES.items():
        if only and only != key:
            continue
        ps = plans(make(W))
        calls = {}
        for which, p in ps.items():
            calls[which], info, keep = entries(p, nc, np.random.default_rng(0))  # the same inputs for both plans
            calls[which]["_info"], calls[which]["_keep"] = info, keep
        r = {"case": name, "cells": nc, "n_nodes": ps["front"].n_nodes, "n_el": ps["front"].n_el, "front_width": ps["front"].front_width,
             "load_kernel": {w: p.load_kernel for w, p in ps.items()}}
        for entry in ("response", "second", "canonical"):
            ts = {w: [] for w in ps}
            for rep in range(reps + 1):  # the first round is the warm-up
                for w in ps:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    calls[w][entry]()
                    torch.cuda.synchronize()
                    if rep:
                        ts[w].append(time.perf_counter() - t0)
            for w in ps:
                assert int((calls[w]["_info"] != 0).sum()) == 0
                r[f"{entry}_{w}_s"] = float(np.median(ts[w]))
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def profile_leg(nc, reps, only, entry):
    import torch

    from hommx_amd import workloads as W

    name, make = CASES[only]
    p = plans(make(W))["front"]
    call, info, keep = entries(p, nc, np.random.default_rng(0))
    for _ in range(reps + 1):
        call[entry]()
    torch.cuda.synchronize()
    assert int((info != 0).sum()) == 0


def merge(doc, only, entry, stats_csv, api_calls):
    rows = list(csv.DictReader(open(stats_csv)))
    def kernel_of(full):  # the name up to its template arguments: "k_mesh_front" is a prefix of "k_mesh_front_rhs"
        return next((k for k in KERNELS if f"{k}<" in full or full.endswith(k) or f"{k}(" in full), None)

    for r in doc["results"]:
        if r["case"] == CASES[only][0]:
            acc = {}
            for row in rows:
                k = kernel_of(row["Name"])
                if k:
                    acc[k] = acc.get(k, 0.0) + float(row["TotalDurationNs"]) * 1e-9 / api_calls
            r[f"{entry}_front_kernels_s"] = acc
    doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats (a run of its own per case and entry): TotalDurationNs per API call"
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/mesh_front_loads_bench.json")
    ap.add_argument("--case", choices=tuple(CASES), default=None)
    ap.add_argument("--profile-leg", choices=("response", "second", "canonical"), default=None, help="one entry of the frontal plan alone, no JSON")
    ap.add_argument("--merge-kernel-stats", nargs=2, metavar=("ENTRY", "CSV"), default=None, help="kernel stats of a traced --profile-leg ENTRY run")
    a = ap.parse_args()
    if a.profile_leg:
        return profile_leg(a.cells, a.reps, a.case, a.profile_leg)
    if a.merge_kernel_stats:
        doc = merge(json.load(open(a.out)), a.case, a.merge_kernel_stats[0], a.merge_kernel_stats[1], a.reps + 1)
    else:
        doc = {"tool": "tools/bench_mesh_loads.py", "reps": a.reps, "statistic": "median wall time after one warm-up call, the plans alternating",
               "results": measure(a.cells, a.reps, a.case)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
