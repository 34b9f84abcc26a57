"""Cost of the derivatives of A_H with respect to the stratification M (hommx_stratification_sensitivity_source[_device]) on
the C2 shape (8,192 cells, 32^2 scalar Poisson, the TwoPhase inclusion, M a rotation by 0.3 + x0) and the C4 shape (256 cells, 16^3
isotropic elasticity, the TwoPhase fibre, M of the C5 map), beside the yardsticks of the same batch in the same run: the derivatives along
coefficient directions (hommx_sensitivity_source: two directions, and d^2 of them -- eight in 3D, the most a call takes) and the
finite-difference route the call replaces (2 d^2 tensor solves).

    python tools/bench_strat_sens.py [--reps 7] [--out profiles/strat_sens_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_strat_sens.py --case C2 --profile-leg --reps 3
    python tools/bench_strat_sens.py --case C2 --merge-kernel-stats DIR/.../run_kernel_stats.csv [--out profiles/strat_sens_bench.json]

Per case, the median wall time after one warm-up call of plan.stratification_sensitivities (host entry: the two-phase stream and M go in,
dA_dM comes back) and plan.stratification_sensitivities_device (everything resident; dA_dM, and grad_M alone).  --profile-leg runs the
device entry (dA_dM) of one case alone, so that a rocprofv3 trace of that run holds the kernels of the corrector route, the expansion of
the stream and k_sens_strat, and nothing else; --merge-kernel-stats adds k_sens_strat against the sum of the route's kernels from that
trace."""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_sens import median_time, phase_directions  # noqa: E402


def cases():
    from hommx_amd import workloads as W

    msh2, mask2, values2 = W.c2_inclusion_two_phase()
    ang = 0.3 + msh2.cell_midpoints()[:len(values2), 0]
    M2 = np.ascontiguousarray(np.moveaxis(np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]), -1, 0))
    msh4, mask4, values4, _ = W.c4_two_phase(cells=np.arange(256))
    M4 = W.c5_theta_transpose(msh4.cell_midpoints()[:256])
    return [("C2: 8192 cells, 32^2 Poisson with M", 2, 32, "poisson", mask2, values2, M2),
            ("C4: 256 cells, 16^3 elasticity with M", 3, 16, "elasticity", mask4, values4, M4)]


def measure(reps, only, profile_leg):
    import torch

    from hommx_amd import MicroCellPlan, _lib
    from hommx_amd.batch import CoefStream

    out = []
    for name, dim, n, kind, mask, values, M in cases():
        if only and only not in name:
            continue
        p = MicroCellPlan(dim, n, kind)
        nc, t = values.shape[0], p.t
        assert M.shape == (nc, dim, dim)
        stream = CoefStream.two_phase(mask, values)
        rng = np.random.default_rng(0)
        w = rng.standard_normal((nc, t, t))
        dirs2 = phase_directions(mask.astype(float), p.n_comp)[:2]
        ndd = min(dim * dim, _lib.SENS_MAX_DIRS)
        dirs_dd = np.concatenate([dirs2, rng.standard_normal((ndd - 2,) + dirs2.shape[1:])])
        dev = torch.device("cuda", p.device)
        keep = []

        def upload(a):
            keep.append(torch.from_numpy(np.array(a)).to(dev))
            return keep[-1].data_ptr()

        src = stream.coef_source(upload)
        d_M, d_w, d_dirs = upload(M), upload(w), upload(dirs_dd)
        dAdM = torch.empty((nc, dim, dim, t, t), dtype=torch.float64, device=dev)
        gM = torch.empty((nc, dim, dim), dtype=torch.float64, device=dev)
        dA = torch.empty((nc, ndd, t, t), dtype=torch.float64, device=dev)
        A = torch.empty((nc, t, t), dtype=torch.float64, device=dev)
        info = torch.empty(nc, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        out_kw = dict(A_ptr=A.data_ptr(), info_ptr=info.data_ptr(), stream=s)
        strat_device = lambda: p.stratification_sensitivities_device(nc, src, d_M, dAdM.data_ptr(), **out_kw)
        r = {"case": name, "cells": nc, "kernel_route": p.kernel, "corrector_kernel": p.corrector_kernel}
        r["strat_sens_device_s"] = median_time(strat_device, reps)
        assert int((info != 0).sum()) == 0
        if not profile_leg:
            r["strat_sens_grad_only_device_s"] = median_time(
                lambda: p.stratification_sensitivities_device(nc, src, d_M, None, d_w, gM.data_ptr(), **out_kw), reps)
            r["strat_sens_host_s"] = median_time(lambda: p.stratification_sensitivities(stream, M), reps)
            for nd, key in ((2, "sensitivities_2_dirs"), (ndd, f"sensitivities_{ndd}_dirs")):
                r[key + "_device_s"] = median_time(lambda: p.sensitivities_device(nc, src, d_M, nd, d_dirs, False, dA.data_ptr(), **out_kw), reps)
                r[key + "_host_s"] = median_time(lambda: p.sensitivities(stream, M, directions=dirs_dd[:nd]), reps)
            r["tensor_solve_host_s"] = median_time(lambda: stream.solve(p, M), reps)
            r["finite_difference_route_host_s"] = 2 * dim * dim * r["tensor_solve_host_s"]
            r["finite_difference_route"] = f"{2 * dim * dim} tensor solves of the batch (central differences along every E_ab), host entry"
        out.append(r)
        print(", ".join(f"{k} {v * 1e3:.2f} ms" if k.endswith("_s") else f"{k}: {v}" for k, v in r.items()), flush=True)
        del p
    return out


def merge(res, stats_csv, only, api_calls):
    """k_sens_strat against the corrector solve of the same chunks: every other kernel of the library in the trace but the expansion of
    the stream (the uploads of this script are not the library's)."""
    rows = list(csv.DictReader(open(stats_csv)))
    total = lambda pick: sum(float(r["TotalDurationNs"]) for r in rows if pick(r["Name"]))
    sens = total(lambda k: "k_sens_strat" in k)
    expand = total(lambda k: "expand" in k)
    ours = lambda k: "hommx::" in k and "k_sens_strat" not in k and "expand" not in k
    route = total(ours)
    for r in res:
        if only in r["case"]:
            r["k_sens_strat_s"] = sens * 1e-9 / api_calls
            r["corrector_kernels_s"] = route * 1e-9 / api_calls
            r["expand_kernel_s"] = expand * 1e-9 / api_calls
            r["k_sens_strat_over_corrector_kernels"] = sens / route
            r["corrector_kernel_names"] = sorted({r2["Name"].split("(")[0][:80] for r2 in rows if ours(r2["Name"])})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/strat_sens_bench.json")
    ap.add_argument("--case", default=None, help="only the cases whose name contains this")
    ap.add_argument("--profile-leg", action="store_true", help="the device entry (dA_dM) alone, no JSON: the run to trace")
    ap.add_argument("--merge-kernel-stats", default=None, help="kernel stats CSV of a traced --profile-leg run of --case (with its --reps)")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        doc = json.load(open(a.out))
        doc["results"] = merge(doc["results"], a.merge_kernel_stats, a.case, a.reps + 1)
        doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats (a run of its own per case, no counters): TotalDurationNs per API call"
    else:
        doc = {"tool": "tools/bench_strat_sens.py", "reps": a.reps, "statistic": "median wall time after one warm-up call",
               "results": measure(a.reps, a.case, a.profile_leg)}
        if a.profile_leg:
            return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
