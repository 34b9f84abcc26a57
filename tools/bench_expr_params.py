"""Cost of the parameter derivatives of an expression coefficient (hommx_expand_tangents, HOMMX_DIRS_PARAMETERS) on
the headline batch: 8,192 cells of 32^2 scalar Poisson, A = 1.1 + x[0] + p[0] sin(2 pi y[0]) + p[1] cos(2 pi y[1]), two parameters.

    python tools/bench_expr_params.py [--reps 5] [--out profiles/expr_params_bench.json]

Median wall time after one warm-up call of
  (a) the tangent pass alone (expand_tangents_device: value stream + two tangent streams; the tangents alone) against the value pass
      alone (expand_device), everything resident;
  (b) plan.sensitivities(stream, directions="parameters") against plan.sensitivities(stream, directions=<the same two directions as
      per-cell host arrays>, per_cell=True), host entries, and the same pair through the device entries with everything resident;
  (c) PoissonHMM.tensor_derivatives() against tensor_derivatives(directions=[two callables]) on a 64 x 64 macro mesh (8,192 cells).
The second legs of (b) and (c) are the routes a coefficient without named parameters has to take; this change does not touch them."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TEXT = "1.1 + x[0] + p[0]*sin(2*pi*y[0]) + p[1]*cos(2*pi*y[1])"
P = [0.5, 0.25]
N_MACRO, N_MICRO = 64, 32  # 2 * 64^2 = 8,192 macro cells


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


def measure(reps):
    import torch

    from hommx_amd import MicroCellPlan, hmm, mesh as Mm
    from hommx_amd.batch import CoefStream

    A = hmm.Expression(TEXT, p=P)
    msh, micro = Mm.create_unit_square(N_MACRO, N_MACRO), Mm.create_unit_square(N_MICRO, N_MICRO)
    x = msh.cell_midpoints()
    nc = x.shape[0]
    bary, w = hmm.micro_quadrature(2, A.degree)
    yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, micro.cell_vertices()))
    p = MicroCellPlan(2, N_MICRO, "poisson")
    stream = CoefStream.program(yq, w, *A.program(), A.n_comp, x, n_params=A.n_params)
    r = {"cells": nc, "n_micro": N_MICRO, "expression": TEXT, "p": P, "degree": A.degree, "n_q": int(len(w)), "n_ops": int(A.program()[0].shape[0]),
         "kernel_route": p.kernel, "corrector_kernel": p.corrector_kernel}
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    src = stream.coef_source(upload)
    s = torch.cuda.current_stream(dev).cuda_stream
    t = p.t
    # (a) the passes alone
    d_coef = torch.empty((nc, p.n_el), dtype=torch.float64, device=dev)
    d_dirs = torch.empty((nc, 2, p.n_el), dtype=torch.float64, device=dev)
    r["value_pass_s"] = median_time(lambda: p.expand_device(nc, src, d_coef.data_ptr(), s), reps)
    r["tangent_pass_with_values_s"] = median_time(lambda: p.expand_tangents_device(nc, src, d_coef.data_ptr(), d_dirs.data_ptr(), s), reps)
    r["tangent_pass_alone_s"] = median_time(lambda: p.expand_tangents_device(nc, src, None, d_dirs.data_ptr(), s), reps)
    r["tangent_over_value_pass"] = r["tangent_pass_with_values_s"] / r["value_pass_s"]
    # (b) the first derivatives
    dirs = d_dirs.cpu().numpy()  # the same two directions as per-cell host arrays (268 MB)
    r["direction_stream_MB"] = dirs.nbytes / 1e6
    r["sensitivities_parameters_host_s"] = median_time(lambda: p.sensitivities(stream, directions="parameters"), reps)
    r["sensitivities_per_cell_arrays_host_s"] = median_time(lambda: p.sensitivities(stream, directions=dirs, per_cell=True), reps)
    dA = torch.empty((nc, 2, t, t), dtype=torch.float64, device=dev)
    A_eff = torch.empty((nc, t, t), dtype=torch.float64, device=dev)
    info = torch.empty(nc, dtype=torch.int32, device=dev)
    out = dict(A_ptr=A_eff.data_ptr(), info_ptr=info.data_ptr(), stream=s)
    r["sensitivities_parameters_device_s"] = median_time(lambda: p.sensitivities_device(nc, src, None, 2, None, "parameters", dA.data_ptr(), **out), reps)
    got = dA.cpu().numpy()
    r["sensitivities_per_cell_arrays_device_s"] = median_time(
        lambda: p.sensitivities_device(nc, src, None, 2, d_dirs.data_ptr(), True, dA.data_ptr(), **out), reps)
    assert int((info != 0).sum()) == 0 and np.array_equal(dA.cpu().numpy(), got)  # the two routes give the same bits
    r["host_speedup_over_per_cell_arrays"] = r["sensitivities_per_cell_arrays_host_s"] / r["sensitivities_parameters_host_s"]
    print(json.dumps(r, indent=1), flush=True)
    del keep[:], d_coef, d_dirs, dirs
    # (c) the solver class
    h = hmm.PoissonHMM(msh, A, lambda x: 1.0 + x[0], micro, 0.01)
    callables = [lambda x, y: np.sin(2 * np.pi * y[0]) + 0.0 * x[0], lambda x, y: np.cos(2 * np.pi * y[1]) + 0.0 * x[0]]
    a = h.tensor_derivatives()
    b = h.tensor_derivatives(directions=callables)
    r["hmm_max_rel_difference_of_dA"] = float(np.abs(a.dA - b.dA).max() / np.abs(b.dA).max())
    r["hmm_tensor_derivatives_parameters_s"] = median_time(lambda: h.tensor_derivatives(), reps)
    r["hmm_tensor_derivatives_callables_s"] = median_time(lambda: h.tensor_derivatives(directions=callables), reps)
    r["hmm_speedup_over_callables"] = r["hmm_tensor_derivatives_callables_s"] / r["hmm_tensor_derivatives_parameters_s"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/expr_params_bench.json")
    a = ap.parse_args()
    doc = {"tool": "tools/bench_expr_params.py", "reps": a.reps, "statistic": "median wall time after one warm-up call",
           "baselines": "the per-cell host arrays of (b) and the callables of (c) are routes this change does not touch, measured in the same process",
           "results": measure(a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
