"""Cost of the second derivatives of A_H along coefficient directions (hommx_second_sensitivity_source[_device]) on the
C2 shape (8,192 cells, 32^2 scalar Poisson, the TwoPhase inclusion, 2 directions: d / d outside, d / d inside) and the C4 shape (256
cells, 16^3 isotropic elasticity, the TwoPhase fibre, 4 directions: both Lame parameters of both phases), against the finite-difference
route to the same Hessian: 2 n_dirs calls of hommx_sensitivity_source_device, the gradients at coef +- h dir_b.

    python tools/bench_sens2.py [--reps 7] [--out profiles/sens2_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_sens2.py --case C2 --profile-leg --reps 3
    python tools/bench_sens2.py --case C2 --merge-kernel-stats DIR/.../run_kernel_stats.csv [--out profiles/sens2_bench.json]

Per case, the median wall time after one warm-up call of plan.second_sensitivities (host entry: the two-phase stream and the shared
directions go in, d2A and dA come back) and plan.second_sensitivities_device (everything resident), and of the 2 n_dirs gradient calls.
The loads of one direction take t n_el t doubles of plan scratch per cell (7 MB at 16^3 elasticity), so the default HOMMX_RECON_MEM_MB
holds fewer cells per chunk than the batch has: the C4 case is measured at the default and at a setting that holds all of them (the
variable is read when a plan is created).  --profile-leg runs the device entry of one case alone, so that a rocprofv3 trace of that run
holds the kernels of the call and nothing else; --merge-kernel-stats adds the share of k_sens2_loads and k_sens2 from that trace."""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_sens import cases, median_time, phase_directions  # noqa: E402  (the shapes and the protocol of the first derivatives)


def chunk_cells(p, nc, mem_mb):
    """Cells per chunk of the device entry: recon_chunk of api.hip with the bytes a second-derivative chunk holds per cell -- two blocks
    of t correctors (and the chi^xi slot of cells too large for LDS), the loads of one direction, on a fused 2D plan its factor record and
    refinement scratch."""
    bs = 1 if p.kind.startswith("poisson") else p.dim
    ndof, t = p.n_nodes * bs, p.t
    per = 8 * ndof * (2 * t + (1 if 8 * ndof > 150 * 1024 else 0)) + 8 * t * p.n_el * t
    if p.corrector_kernel == "fused2d_subst":
        nb, n = (16 if p.n_micro <= 16 else 32), p.n_micro
        per += 8 * (4 * nb + 8 + (n - 1) * (nb * nb + 4 * nb) + nb * nb) + 8 * 10 * n * n
    return max(1, min(nc, (mem_mb << 20) // per)), per


def measure(reps, only, profile_leg):
    import torch

    from hommx_amd import MicroCellPlan
    from hommx_amd.batch import CoefStream

    out = []
    for name, dim, n, kind, mask, values in cases():
        if only and only not in name:
            continue
        nc = values.shape[0]
        default_mb = int(os.environ.get("HOMMX_RECON_MEM_MB", "0")) or 1024
        settings = [default_mb]
        probe = MicroCellPlan(dim, n, kind)
        chunk, per = chunk_cells(probe, nc, default_mb)
        del probe
        if chunk < nc and not profile_leg:
            settings.append((nc * per >> 20) + 64)  # every cell in one chunk
        for mb in settings:
            os.environ["HOMMX_RECON_MEM_MB"] = str(mb)
            p = MicroCellPlan(dim, n, kind)
            t = p.t
            stream = CoefStream.two_phase(mask, values)
            dirs = phase_directions(mask.astype(float), p.n_comp)
            nd = dirs.shape[0]
            dev = torch.device("cuda", p.device)
            keep = []

            def upload(a):
                keep.append(torch.from_numpy(np.array(a)).to(dev))
                return keep[-1].data_ptr()

            src = stream.coef_source(upload)
            d_dirs = upload(dirs)
            d2A = torch.empty((nc, nd, nd, t, t), dtype=torch.float64, device=dev)
            dA = torch.empty((nc, nd, t, t), dtype=torch.float64, device=dev)
            A = torch.empty((nc, t, t), dtype=torch.float64, device=dev)
            info = torch.empty(nc, dtype=torch.int32, device=dev)
            s = torch.cuda.current_stream(dev).cuda_stream
            second = lambda: p.second_sensitivities_device(nc, src, None, nd, d_dirs, d2A.data_ptr(), False, dA.data_ptr(), A.data_ptr(),
                                                           info.data_ptr(), stream=s)
            first = lambda: p.sensitivities_device(nc, src, None, nd, d_dirs, False, dA.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(),
                                                   stream=s)

            def differences():  # the gradients at coef +- h dir_b: 2 n_dirs calls (the perturbed values cost what these cost)
                for _ in range(2 * nd):
                    first()

            r = {"case": name, "cells": nc, "n_dirs": nd, "kernel_route": p.kernel, "corrector_kernel": p.corrector_kernel,
                 "load_kernel": p.load_kernel, "recon_mem_mb": mb, "bytes_per_cell_of_a_chunk": per, "cells_per_chunk": chunk_cells(p, nc, mb)[0]}
            r["second_sensitivities_device_s"] = median_time(second, reps)
            assert int((info != 0).sum()) == 0
            if not profile_leg:
                r["second_sensitivities_host_s"] = median_time(lambda: p.second_sensitivities(stream, directions=dirs, first=True), reps)
                r["sensitivities_device_s"] = median_time(first, reps)
                r["finite_difference_route_device_s"] = median_time(differences, reps)
                r["exact_over_finite_differences"] = r["second_sensitivities_device_s"] / r["finite_difference_route_device_s"]
            out.append(r)
            print(", ".join(f"{k} {v * 1e3:.2f} ms" if k.endswith("_s") else f"{k}: {v}" for k, v in r.items()), flush=True)
            p.close()
            del p, keep
        os.environ["HOMMX_RECON_MEM_MB"] = str(default_mb)
    return out


def merge(res, stats_csv, only, api_calls):
    """k_sens2_loads and k_sens2 against every other kernel of the library in the trace of one case (the canonical pass, the load solves,
    k_sens, the expansion of the stream); the uploads of this script are not the library's."""
    rows = list(csv.DictReader(open(stats_csv)))
    total = lambda pick: sum(float(r["TotalDurationNs"]) for r in rows if pick(r["Name"]))
    loads = total(lambda k: "k_sens2_loads" in k)
    sens2 = total(lambda k: "k_sens2<" in k)
    rest = total(lambda k: "hommx::" in k and "k_sens2" not in k)
    for r in [x for x in res if only in x["case"]][:1]:  # the leg runs at the default chunk: the first entry of the case
        r["k_sens2_loads_s"] = loads * 1e-9 / api_calls
        r["k_sens2_s"] = sens2 * 1e-9 / api_calls
        r["other_kernels_s"] = rest * 1e-9 / api_calls
        r["new_kernels_share"] = (loads + sens2) / (loads + sens2 + rest)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/sens2_bench.json")
    ap.add_argument("--case", default=None, help="only the cases whose name contains this")
    ap.add_argument("--profile-leg", action="store_true", help="the device entry alone at the default chunk, no JSON: the run to trace")
    ap.add_argument("--merge-kernel-stats", default=None, help="kernel stats CSV of a traced --profile-leg run of --case (with its --reps)")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        doc = json.load(open(a.out))
        doc["results"] = merge(doc["results"], a.merge_kernel_stats, a.case, a.reps + 1)
        doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats (a run of its own per case, no counters): TotalDurationNs per API call"
    else:
        doc = {"tool": "tools/bench_sens2.py", "reps": a.reps, "statistic": "median wall time after one warm-up call",
               "results": measure(a.reps, a.case, a.profile_leg)}
        if a.profile_leg:
            return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
