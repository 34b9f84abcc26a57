"""Cost of user-supplied polarisation loads (hommx_loads_source[_device]) on the C2 shape (8,192 cells, 32^2 scalar
Poisson, the TwoPhase inclusion) and on 256 cells of the C4 shape (16^3 isotropic elasticity, the TwoPhase fibre), one load shared by all
cells (a thermal eigenstress: material(phase) applied to one unit strain).

    python tools/bench_loads.py [--reps 7] [--fused-loads 0|1] [--out profiles/loads_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_loads.py --case C2 --profile-leg --reps 3
    python tools/bench_loads.py --case C2 --merge-kernel-stats DIR/.../run_kernel_stats.csv [--out profiles/loads_bench.json]

Per case, the median wall time after one warm-up call of
    P_eff alone (device and host entry): the canonical correctors of every chunk and k_polar -- next to the derivative of A_H along one
        direction (hommx_sensitivity_source), the same correctors and one contraction;
    the response (device entry, statistics and energy, no fields): one more corrector pass on the overridden load rows and k_load_stats --
        next to the reconstruction (statistics only) and the corrector call (hommx_solve_batch_correctors, host entry) of the same batch.
--fused-loads sets HOMMX_FUSED_LOADS before the plans are created: 0 is the plane elimination for the load solve of the fused 2D plan (the
yardstick of DESIGN.md 4.10), 1 / default the substitution on the factor records (k_fused2d_subst_rhs); `load_kernel` in the JSON is the route
taken.  --profile-leg runs the response's device entry of one case alone, so that a rocprofv3 trace of that run holds the kernels of both
corrector passes, k_polar, k_assemble_loads (blocked load pass) or k_fused2d_subst_rhs, and k_load_stats; --merge-kernel-stats adds their
times per API call and their algorithmic bytes."""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cases():
    from hommx_amd import workloads as W

    _, mask2, values2 = W.c2_inclusion_two_phase()
    _, mask4, values4, _ = W.c4_two_phase(cells=np.arange(256))
    return [("C2: 8192 cells, 32^2 Poisson", 2, 32, "poisson", mask2, values2), ("C4: 256 cells, 16^3 elasticity", 3, 16, "elasticity", mask4, values4)]


def eigenstress(mask, kind, t):
    """P[1, n_el, t]: material(phase) e_0 with phase values 1 / 10 (Lame: lambda = mu) -- the stress of a unit strain in direction 0."""
    c = np.where(np.asarray(mask, bool), 10.0, 1.0)
    P = np.zeros((1, len(c), t))
    if kind == "poisson":
        P[0, :, 0] = c
    else:
        d = 3
        P[0, :, :d] = c[:, None]  # lambda tr(e_0)
        P[0, :, 0] += 2.0 * c
    return P


def median_time(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def measure(reps, only, profile_leg):
    import torch

    from hommx_amd import MicroCellPlan
    from hommx_amd.batch import CoefStream

    out = []
    for name, dim, n, kind, mask, values in cases():
        if only and only not in name:
            continue
        p = MicroCellPlan(dim, n, kind)
        nc, t = values.shape[0], p.t
        stream = CoefStream.two_phase(mask, values)
        P = eigenstress(mask, kind, t)
        direction = (1.0 * np.asarray(mask, bool))[None] if p.n_comp == 1 else (np.asarray(mask, bool)[:, None] * np.eye(p.n_comp)[0])[None]
        xi = np.random.default_rng(0).standard_normal((nc, t))
        dev = torch.device("cuda", p.device)
        keep = []

        def upload(a):
            keep.append(torch.from_numpy(np.array(a)).to(dev))
            return keep[-1].data_ptr()

        src = stream.coef_source(upload)
        d_P, d_dir, d_xi = upload(P), upload(direction), upload(xi)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        P_eff, energy, lstats, dA, st, A = new(nc, 1, t), new(nc, 1, 1), new(nc, 1, t + 2), new(nc, 1, t, t), new(nc, 2 * t + 3), new(nc, t, t)
        info = torch.empty(nc, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        r = {"case": name, "cells": nc, "n_loads": 1, "kernel_route": p.kernel, "corrector_kernel": p.corrector_kernel,
             "load_kernel": p.load_kernel}
        response = lambda: p.loads_device(nc, src, None, 1, d_P, P_eff.data_ptr(), False, A.data_ptr(), info.data_ptr(), energy.data_ptr(),
                                          lstats.data_ptr(), stream=s)
        if not profile_leg:
            r["p_eff_device_s"] = median_time(lambda: p.loads_device(nc, src, None, 1, d_P, P_eff.data_ptr(), False, A.data_ptr(), info.data_ptr(),
                                                                     stream=s), reps)
            r["p_eff_host_s"] = median_time(lambda: p.loads(stream, P), reps)
            r["sensitivity_one_direction_device_s"] = median_time(
                lambda: p.sensitivities_device(nc, src, None, 1, d_dir, False, dA.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(), stream=s), reps)
            r["reconstruct_stats_device_s"] = median_time(
                lambda: p.reconstruct_source_device(nc, src, None, d_xi, st.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(), stream=s), reps)
        r["response_device_s"] = median_time(response, reps)
        assert int((info != 0).sum()) == 0
        if not profile_leg:
            r["response_host_s"] = median_time(lambda: p.loads(stream, P, response=True), reps)
            if dim == 3:  # the corrector call of the tree route (host entry: the correctors come back, 151 MB at this size)
                coef = values[:, np.asarray(mask).astype(int)]
                r["correctors_host_s"] = median_time(lambda: p.solve(coef, return_correctors=True), max(1, reps // 3))
            r["levin_against_direct"] = float((P_eff[:, 0] - lstats[:, 0, :t]).abs().max() / P_eff.abs().max())
        out.append(r)
        print(", ".join(f"{k} {v * 1e3:.2f} ms" if k.endswith("_s") else f"{k}: {v}" for k, v in r.items()), flush=True)
        del p
    return out


def merge(res, stats_csv, only, api_calls):
    """The three load kernels against the corrector kernels of the same call, per API call, with their algorithmic bytes."""
    rows = list(csv.DictReader(open(stats_csv)))
    total = lambda pick: sum(float(r["TotalDurationNs"]) for r in rows if pick(r["Name"]))
    mine = ("k_polar", "k_assemble_loads", "k_load_stats", "k_fused2d_subst_rhs")
    ours = lambda k: "hommx::" in k and not any(m in k for m in mine) and "expand" not in k
    for r in res:
        if only in r["case"]:
            dim, n, t, bs, nc = (2, 32, 2, 1, r["cells"]) if "C2" in r["case"] else (3, 16, 6, 3, r["cells"])
            n_el, ndof, n_comp = (2 if dim == 2 else 6) * n**dim, bs * n**dim, 1 if dim == 2 else 2
            # unique bytes: k_polar reads t correctors and P (shared) and writes t numbers; k_assemble_loads reads P and writes t rows of Brhs;
            # k_load_stats reads the coefficient and P per load and, in the pass of load l, the correctors 0 .. l: one corrector at the one
            # load of this benchmark (n_loads (n_loads + 1) / 2 corrector reads per cell in general)
            bytes_ = {"k_polar": 8.0 * nc * (t * ndof + t) + 8.0 * n_el * t, "k_assemble_loads": 8.0 * nc * t * ndof + 8.0 * n_el * t,
                      "k_load_stats": 8.0 * nc * (ndof + n_el * n_comp + t + 3) + 8.0 * n_el * t,
                      # the record's block inverses four times (the last one once), the load and one corrector row
                      "k_fused2d_subst_rhs": 8.0 * nc * ((4 * (n - 1) - 2) * n * n + ndof) + 8.0 * n_el * t if dim == 2 else 0.0}
            for m in mine:
                r[m + "_s"] = total(lambda k: m in k) * 1e-9 / api_calls
                r[m + "_bytes"] = bytes_[m]
            r["corrector_kernels_s"] = total(ours) * 1e-9 / api_calls
            r["corrector_kernel_names"] = sorted({r2["Name"].split("(")[0][:80] for r2 in rows if ours(r2["Name"])})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/loads_bench.json")
    ap.add_argument("--fused-loads", choices=("0", "1"), default=None, help="HOMMX_FUSED_LOADS for the plans of this run (default: unset)")
    ap.add_argument("--case", default=None, help="only the cases whose name contains this")
    ap.add_argument("--profile-leg", action="store_true", help="the device entry of the response alone, no JSON: the run to trace")
    ap.add_argument("--merge-kernel-stats", default=None, help="kernel stats CSV of a traced --profile-leg run of --case (with its --reps)")
    a = ap.parse_args()
    if a.fused_loads is not None:
        os.environ["HOMMX_FUSED_LOADS"] = a.fused_loads
    if a.merge_kernel_stats:
        doc = json.load(open(a.out))
        doc["results"] = merge(doc["results"], a.merge_kernel_stats, a.case, a.reps + 1)
        doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats (a run of its own per case, no counters): TotalDurationNs per API call"
    else:
        doc = {"tool": "tools/bench_loads.py", "reps": a.reps, "statistic": "median wall time after one warm-up call",
               "results": measure(a.reps, a.case, a.profile_leg)}
        if a.profile_leg:
            return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
