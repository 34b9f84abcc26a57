"""Cost split of the HMM reconstruction (hommx_reconstruct_batch_device): the corrector solve against the reconstruction
kernel k_recon, on the C2 shape (8,192 cells, 32^2 scalar Poisson, inclusion element stream) and the C4 shape (256 cells, 16^3 isotropic
elasticity, fibre element stream); the C2 shape at 8^2 as well (the NB = 16 kernels of the fused family).  `corrector_kernel` in the JSON
is the route the corrector solve took (hommx_plan_corrector_kernel_name; HOMMX_FUSED_CORR=0 / HOMMX_MF_CORR=0 for the A/B runs).

    python tools/bench_reconstruct.py [--reps 7] [--out profiles/recon_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_reconstruct.py --reps 3 --no-json
    python tools/bench_reconstruct.py --merge-kernel-stats DIR/.../run_kernel_stats.csv [--out profiles/recon_bench.json]
    python tools/bench_reconstruct.py --form two_phase [--regions] [--out profiles/recon_source_bench.json]

Per case, the median wall time after one warm-up call of: hommx_solve_batch_correctors (host pointers: the only form it has; the
correctors of the whole batch cross PCIe), hommx_reconstruct_batch_device with statistics only, and with fields.  The device entry takes
torch tensors already resident.  --merge-kernel-stats adds the time of k_recon alone from a separate rocprofv3 run, and its algorithmic
bytes/s: correctors and coef read once, xi / M read once, stats (and fields) written once.

--form two_phase: the C2 shape through hommx_reconstruct_source: PoissonHMM.reconstruct() end to end with the TwoPhase
inclusion coefficient (the macro field is a fixed smooth function, no macro solve), the plan's host entry given the two-phase stream and
given the sampled element stream (hommx_reconstruct_batch), every figure with its spread over the repetitions.  --regions adds the same
legs with the two phases as regions; under rocprofv3 the k_recon<..., true> rows are the instantiations with regions."""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12  # MI355X_MICROARCH.md: datasheet, measured device-to-device copy


def cases():
    from hommx_amd import workloads as W

    _, coef2, _ = W.c2_inclusion(nx=64, n=32)
    _, coef2s, _ = W.c2_inclusion(nx=64, n=8)
    _, mask, values, _ = W.c4_two_phase(cells=np.arange(256))
    coef4 = values[:, mask.astype(int), :]
    return [("C2: 8192 cells, 32^2 Poisson", 2, 32, "poisson", coef2, "k_recon<2, 0, false"),
            ("C2 at 8^2: 8192 cells, 8^2 Poisson", 2, 8, "poisson", coef2s, "k_recon<2, 0, false"),  # the NB = 16 kernels of the fused family
            ("C4: 256 cells, 16^3 elasticity", 3, 16, "elasticity", coef4, "k_recon<3, 2, false")]


def bytes_per_cell(p, fields):
    bs = 1 if p.kind.startswith("poisson") else p.dim
    ndof = p.n_nodes * bs
    b = 8 * (p.t * ndof + p.n_el * p.n_comp + p.t + (2 * p.t + 3))
    return b + (8 * 2 * p.n_el * p.t if fields else 0)


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


def measure(reps, only=None):
    import torch

    from hommx_amd import MicroCellPlan

    out = []
    for name, dim, n, kind, coef, kname in cases():
        if only and only not in name:
            continue
        p = MicroCellPlan(dim, n, kind)
        nc = coef.shape[0]
        t = p.t
        rng = np.random.default_rng(0)
        xi = rng.standard_normal((nc, t))
        dev = torch.device("cuda", p.device)
        dc, dx = torch.from_numpy(np.ascontiguousarray(coef)).to(dev), torch.from_numpy(xi).to(dev)
        st = torch.empty((nc, 2 * t + 3), dtype=torch.float64, device=dev)
        A = torch.empty((nc, t, t), dtype=torch.float64, device=dev)
        info = torch.empty(nc, dtype=torch.int32, device=dev)
        fs = torch.empty((nc, p.n_el, t), dtype=torch.float64, device=dev)
        fq = torch.empty_like(fs)
        s = torch.cuda.current_stream(dev).cuda_stream
        t_corr = median_time(lambda: p.solve(coef, return_correctors=True), reps)
        t_stats = median_time(lambda: p.reconstruct_device(nc, dc.data_ptr(), None, dx.data_ptr(), st.data_ptr(), None, None, A.data_ptr(),
                                                           info.data_ptr(), s), reps)
        t_fields = median_time(lambda: p.reconstruct_device(nc, dc.data_ptr(), None, dx.data_ptr(), st.data_ptr(), fs.data_ptr(),
                                                            fq.data_ptr(), A.data_ptr(), info.data_ptr(), s), reps)
        assert int((info != 0).sum()) == 0
        out.append({"case": name, "cells": nc, "kernel_route": p.kernel, "corrector_kernel": p.corrector_kernel, "correctors_host_s": t_corr,
                    "reconstruct_stats_s": t_stats, "reconstruct_fields_s": t_fields,
                    "alg_bytes_per_cell_stats": bytes_per_cell(p, False), "alg_bytes_per_cell_fields": bytes_per_cell(p, True),
                    "kernel_name_prefix": kname})
        print(f"{name}: correctors (host entry) {t_corr * 1e3:.1f} ms, reconstruct stats {t_stats * 1e3:.1f} ms, "
              f"fields {t_fields * 1e3:.1f} ms", flush=True)
        del p
    return out


def spread(fn, reps):
    """Median, minimum and maximum wall time of `reps` calls after one warm-up call."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def measure_source(reps, regions):
    """C2, 8,192 cells: the host entries (they synchronise before they return) and the solver class."""
    from hommx_amd import MicroCellPlan, hmm, mesh, workloads as W
    from hommx_amd.batch import CoefStream

    msh, mask, values = W.c2_inclusion_two_phase()
    _, coef, _ = W.c2_inclusion()
    p = MicroCellPlan(2, 32, "poisson")
    xi = np.random.default_rng(0).standard_normal((coef.shape[0], 2))
    stream = CoefStream.two_phase(mask, values)
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.001 * (1.0 + 9.0 * x[0]), lambda x: 0.1 + 0.0 * x[0])
    h = hmm.PoissonHMM(msh, tp, lambda x: 1.0, mesh.create_unit_square(32, 32), 0.01)
    x = h.function_space.tabulate_dof_coordinates()
    u = np.sin(2.0 * x[:, 0]) * np.cos(x[:, 1])
    legs = {"reconstruct_batch_sampled": lambda: p.reconstruct(coef, xi),
            "reconstruct_source_two_phase": lambda: p.reconstruct(stream, xi),
            "poisson_hmm_reconstruct": lambda: h.reconstruct(u)}
    if regions:
        legs["reconstruct_source_two_phase_regions"] = lambda: p.reconstruct(stream, xi, regions=True)
        legs["poisson_hmm_reconstruct_regions"] = lambda: h.reconstruct(u, regions=True)
    out = {"case": "C2: 8192 cells, 32^2 Poisson, TwoPhase inclusion", "cells": int(coef.shape[0]), "kernel_route": p.kernel,
           "corrector_kernel": p.corrector_kernel}
    for name, fn in legs.items():
        out[name] = spread(fn, reps)
        print(f"{name}: median {out[name]['median_s'] * 1e3:.1f} ms (min {out[name]['min_s'] * 1e3:.1f}, max {out[name]['max_s'] * 1e3:.1f})", flush=True)
    return [out]


def merge(res, stats_csv):
    rows = list(csv.DictReader(open(stats_csv)))
    for r in res:
        for fields, key in ((False, "stats"), (True, "fields")):
            want = r["kernel_name_prefix"] + (", true>" if fields else ", false>")
            hit = [row for row in rows if want in row["Name"]]
            if not hit:
                continue
            avg_ns = float(hit[0]["AverageNs"])
            nbytes = r["cells"] * r[f"alg_bytes_per_cell_{key}"]
            r[f"k_recon_{key}_s"] = avg_ns * 1e-9
            r[f"k_recon_{key}_alg_TBps"] = nbytes / (avg_ns * 1e-9) / 1e12
            r[f"k_recon_{key}_frac_of_copy"] = nbytes / (avg_ns * 1e-9) / HBM_COPY
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/recon_bench.json")
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--merge-kernel-stats", default=None)
    ap.add_argument("--case", default=None, help="only the cases whose name contains this (the two C2 shapes share one k_recon instantiation: "
                    "profile them in runs of their own before --merge-kernel-stats)")
    ap.add_argument("--form", choices=["sampled", "two_phase"], default="sampled")
    ap.add_argument("--regions", action="store_true", help="with --form two_phase: the legs with the two phases as regions as well")
    a = ap.parse_args()
    if a.form == "two_phase":
        doc = {"tool": "tools/bench_reconstruct.py --form two_phase" + (" --regions" if a.regions else ""), "reps": a.reps,
               "statistic": "median / min / max wall time after one warm-up call", "results": measure_source(a.reps, a.regions)}
    elif a.merge_kernel_stats:
        doc = json.load(open(a.out))
        doc["results"] = merge(doc["results"], a.merge_kernel_stats)
        doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats (separate run, AverageNs per instantiation)"
    else:
        doc = {"tool": "tools/bench_reconstruct.py", "reps": a.reps, "statistic": "median wall time after one warm-up call",
               "hbm_spec_Bps": HBM_SPEC, "hbm_copy_Bps": HBM_COPY, "results": measure(a.reps, a.case)}
    if not a.no_json:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
        print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
