"""Cost of the derivatives of A_H along coefficient directions (hommx_sensitivity_source[_device]) on the C2 shape (8,192
cells, 32^2 scalar Poisson, the TwoPhase inclusion, 2 directions: d / d outside, d / d inside) and the C4 shape (256 cells, 16^3 isotropic
elasticity, the TwoPhase fibre, 4 directions: both Lame parameters of both phases), with the reconstruction (statistics only) of the same
batch as the yardstick: both calls form the correctors of every chunk and run one kernel over the elements behind them.

    python tools/bench_sens.py [--reps 7] [--out profiles/sens_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_sens.py --case C2 --profile-leg --reps 3
    python tools/bench_sens.py --case C2 --merge-kernel-stats DIR/.../run_kernel_stats.csv [--out profiles/sens_bench.json]

Per case, the median wall time after one warm-up call of plan.sensitivities (host entry: the two-phase stream and the shared directions go
in, dA comes back) and plan.sensitivities_device (everything resident), and of plan.reconstruct / reconstruct_source_device on the same
stream.  --profile-leg runs the device entry of one case alone, so that a rocprofv3 trace of that run holds the kernels of the corrector
route, the expansion of the stream and k_sens, and nothing else; --merge-kernel-stats adds k_sens against the sum of the route's kernels
from that trace."""

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
    return [("C2: 8192 cells, 32^2 Poisson, 2 directions", 2, 32, "poisson", mask2, values2),
            ("C4: 256 cells, 16^3 elasticity, 4 directions", 3, 16, "elasticity", mask4, values4)]


def phase_directions(mask, n_comp):
    """d / d (value of phase b, component q): the indicator of the phase in that component, in the order of values[2][n_comp]."""
    ind = np.stack([1.0 - mask, 1.0 * mask])
    if n_comp == 1:
        return ind
    return np.stack([ind[b][:, None] * np.eye(n_comp)[q][None, :] for b in range(2) for q in range(n_comp)])


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
        dirs = phase_directions(mask.astype(float), p.n_comp)
        nd = dirs.shape[0]
        xi = np.random.default_rng(0).standard_normal((nc, t))
        dev = torch.device("cuda", p.device)
        keep = []

        def upload(a):
            keep.append(torch.from_numpy(np.array(a)).to(dev))
            return keep[-1].data_ptr()

        src = stream.coef_source(upload)
        d_dirs, d_xi = upload(dirs), upload(xi)
        dA = torch.empty((nc, nd, t, t), dtype=torch.float64, device=dev)
        st = torch.empty((nc, 2 * t + 3), dtype=torch.float64, device=dev)
        A = torch.empty((nc, t, t), dtype=torch.float64, device=dev)
        info = torch.empty(nc, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        sens_device = lambda: p.sensitivities_device(nc, src, None, nd, d_dirs, False, dA.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(),
                                                     stream=s)
        r = {"case": name, "cells": nc, "n_dirs": nd, "kernel_route": p.kernel, "corrector_kernel": p.corrector_kernel}
        r["sensitivities_device_s"] = median_time(sens_device, reps)
        assert int((info != 0).sum()) == 0
        if not profile_leg:
            r["sensitivities_host_s"] = median_time(lambda: p.sensitivities(stream, directions=dirs), reps)
            r["reconstruct_stats_device_s"] = median_time(
                lambda: p.reconstruct_source_device(nc, src, None, d_xi, st.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(), stream=s), reps)
            r["reconstruct_stats_host_s"] = median_time(lambda: p.reconstruct(stream, xi), reps)
        out.append(r)
        print(", ".join(f"{k} {v * 1e3:.2f} ms" if k.endswith("_s") else f"{k}: {v}" for k, v in r.items()), flush=True)
        del p
    return out


def merge(res, stats_csv, only, api_calls):
    """k_sens against the corrector solve of the same chunks: every other kernel of the library in the trace but the expansion of the
    stream (the uploads of this script are not the library's)."""
    rows = list(csv.DictReader(open(stats_csv)))
    total = lambda pick: sum(float(r["TotalDurationNs"]) for r in rows if pick(r["Name"]))
    sens = total(lambda k: "k_sens" in k)
    expand = total(lambda k: "expand" in k)
    ours = lambda k: "hommx::" in k and "k_sens" not in k and "expand" not in k
    route = total(ours)
    for r in res:
        if only in r["case"]:
            r["k_sens_s"] = sens * 1e-9 / api_calls
            r["corrector_kernels_s"] = route * 1e-9 / api_calls
            r["expand_kernel_s"] = expand * 1e-9 / api_calls
            r["k_sens_over_corrector_kernels"] = sens / route
            r["corrector_kernel_names"] = sorted({r2["Name"].split("(")[0][:80] for r2 in rows if ours(r2["Name"])})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/sens_bench.json")
    ap.add_argument("--case", default=None, help="only the cases whose name contains this")
    ap.add_argument("--profile-leg", action="store_true", help="the device entry of the sensitivities alone, no JSON: the run to trace")
    ap.add_argument("--merge-kernel-stats", default=None, help="kernel stats CSV of a traced --profile-leg run of --case (with its --reps)")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        doc = json.load(open(a.out))
        doc["results"] = merge(doc["results"], a.merge_kernel_stats, a.case, a.reps + 1)
        doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats (a run of its own per case, no counters): TotalDurationNs per API call"
    else:
        doc = {"tool": "tools/bench_sens.py", "reps": a.reps, "statistic": "median wall time after one warm-up call",
               "results": measure(a.reps, a.case, a.profile_leg)}
        if a.profile_leg:
            return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
