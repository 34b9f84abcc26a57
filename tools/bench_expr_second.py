"""Cost of the second-order forward mode of an expression coefficient and of the exact Hessian built on it (hommx_expand_second_tangents,
HOMMX_DIRS_PARAMETERS_CURVATURE) on the headline batch: 8,192 cells of 32^2 scalar Poisson, the two-parameter
expression of profiles/expr_params_bench.json made quadratic in one parameter, and a four-parameter one (six launches of the pass).

    python tools/bench_expr_second.py [--reps 9] [--out profiles/expr_second_bench.json]

Everything resident on the device, device entries on the current stream, median wall time around a device synchronise after one warm-up
call of every route; the routes of one comparison alternate inside every repetition.  Per expression:
  (a) the second-order pass (value + tangent + pair streams; the pair streams alone) against the first-order tangent pass and the value pass;
  (b) second_sensitivities_device(..., "parameters", curvature=True) against the same call without the curvature term;
  (c) that call against what a user could do before: central differences of sensitivities_device(..., "parameters"), 2 n_tan further
      gradient calls on the same plan at perturbed parameters -- the comparison of DESIGN 4.13.
The resident workgroups of the second-order kernel at the program's stack depth are computed from the launch geometry (one wave of 64
per block, (depth (1 + P + S) + n_comp S) 512 bytes of dynamic LDS, 160 KiB of LDS and 4 SIMDs per CU, the waves per SIMD of
profiles/coef_program_resource_usage.txt)."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    "two_parameters": ("1.1 + x[0] + p[0]**2*sin(2*pi*y[0]) + p[1]*cos(2*pi*y[1])", [0.5, 0.25]),
    "four_parameters": ("1.1 + x[0] + p[0]**2*sin(2*pi*y[0]) + p[1]*cos(2*pi*y[1]) + p[2]*p[3]*sin(2*pi*y[0])*cos(2*pi*y[1])", [0.5, 0.25, 0.3, 0.3]),
}
N_MACRO, N_MICRO = 64, 32  # 2 * 64^2 = 8,192 macro cells
STEP = 1e-5
WAVES_PER_SIMD = {1: 2, 2: 2}  # k_expand_program2<P> by registers


def median_times(routes, reps):
    """{name: median seconds} of the callables of ``routes``, alternating inside every repetition, after one warm-up call of each."""
    import torch

    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
    return {name: float(np.median(v)) for name, v in ts.items()}


def measure_case(text, values, reps):
    import torch

    from hommx_amd import MicroCellPlan, expr, hmm, mesh as Mm
    from hommx_amd.batch import CoefStream

    A = hmm.Expression(text, p=values)
    msh, micro = Mm.create_unit_square(N_MACRO, N_MACRO), Mm.create_unit_square(N_MICRO, N_MICRO)
    x = msh.cell_midpoints()
    nc, n_tan = x.shape[0], A.n_params
    n_pairs = len(A.pairs)
    bary, w = hmm.micro_quadrature(2, A.degree)
    yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, micro.cell_vertices()))
    p = MicroCellPlan(2, N_MICRO, "poisson")
    depth = max(expr.stack_depths(A.program()[0].tolist()))
    P = min(n_tan, 2)
    S = P * (P + 1) // 2
    lds = (depth * (1 + P + S) + A.n_comp * S) * 64 * 8  # the stack rows, then the sums of the second-order slots
    r = {"cells": nc, "n_micro": N_MICRO, "expression": text, "p": values, "p_degree": A.p_degree, "degree": A.degree, "n_q": int(len(w)),
         "n_ops": int(A.program()[0].shape[0]), "stack_depth": depth, "second_order_launches": 1 if n_tan <= 2 else n_tan * (n_tan - 1) // 2,
         "second_order_dynamic_lds_bytes_per_block": lds,
         "second_order_blocks_per_cu_by_lds": (160 << 10) // lds, "second_order_blocks_per_cu_by_registers": 4 * WAVES_PER_SIMD[P],
         "second_order_resident_blocks_per_cu": min((160 << 10) // lds, 4 * WAVES_PER_SIMD[P]),
         "kernel_route": p.kernel, "corrector_kernel": p.corrector_kernel, "load_kernel": p.load_kernel}
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    def source(B):
        return CoefStream.program(yq, w, *B.program(), B.n_comp, x, n_params=B.n_params).coef_source(upload)

    src = source(A)
    s = torch.cuda.current_stream(dev).cuda_stream
    t = p.t
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    d_coef, d_dirs, d_curv = new(nc, p.n_el), new(nc, n_tan, p.n_el), new(nc, n_pairs, p.n_el)
    # (a) the passes alone
    r.update(median_times({
        "value_pass_s": lambda: p.expand_device(nc, src, d_coef.data_ptr(), s),
        "tangent_pass_with_values_s": lambda: p.expand_tangents_device(nc, src, d_coef.data_ptr(), d_dirs.data_ptr(), s),
        "second_pass_with_values_and_tangents_s": lambda: p.expand_second_tangents_device(nc, src, d_coef.data_ptr(), d_dirs.data_ptr(), d_curv.data_ptr(), s),
        "second_pass_alone_s": lambda: p.expand_second_tangents_device(nc, src, None, None, d_curv.data_ptr(), s),
    }, reps))
    r["second_over_tangent_pass"] = r["second_pass_with_values_and_tangents_s"] / r["tangent_pass_with_values_s"]
    r["second_over_value_pass"] = r["second_pass_with_values_and_tangents_s"] / r["value_pass_s"]
    # (b), (c) the Hessian
    d2A, d2A_along, dA, A_eff = new(nc, n_tan, n_tan, t, t), new(nc, n_tan, n_tan, t, t), new(nc, n_tan, t, t), new(nc, t, t)
    info = torch.empty(nc, dtype=torch.int32, device=dev)
    out = (dA.data_ptr(), A_eff.data_ptr(), info.data_ptr(), s)
    shifted = []
    for k in range(n_tan):
        for sign in (+1.0, -1.0):
            q = np.array(values)
            q[k] += sign * STEP
            shifted.append(source(A.with_parameters(q)))
    sides = [new(nc, n_tan, t, t) for _ in shifted]

    def differences():
        for sk, dk in zip(shifted, sides):
            p.sensitivities_device(nc, sk, None, n_tan, None, "parameters", dk.data_ptr(), A_ptr=A_eff.data_ptr(), info_ptr=info.data_ptr(), stream=s)

    r.update(median_times({
        "second_sensitivities_curvature_s": lambda: p.second_sensitivities_device(nc, src, None, n_tan, None, d2A.data_ptr(), "parameters", *out, curvature=True),
        "second_sensitivities_along_tangents_s": lambda: p.second_sensitivities_device(nc, src, None, n_tan, None, d2A_along.data_ptr(), "parameters", *out),
        "central_differences_of_sensitivities_s": differences,
        "one_sensitivities_call_s": lambda: p.sensitivities_device(nc, src, None, n_tan, None, "parameters", dA.data_ptr(), A_ptr=A_eff.data_ptr(),
                                                                   info_ptr=info.data_ptr(), stream=s),
    }, reps))
    r["gradient_calls_of_the_difference_route"] = len(shifted)
    r["curvature_over_along_tangents"] = r["second_sensitivities_curvature_s"] / r["second_sensitivities_along_tangents_s"]
    r["difference_route_over_exact_route"] = r["central_differences_of_sensitivities_s"] / r["second_sensitivities_curvature_s"]
    # the two routes agree to the accuracy of the difference
    H = d2A.cpu().numpy()
    fd = np.stack([(sides[2 * k].cpu().numpy() - sides[2 * k + 1].cpu().numpy()) / (2 * STEP) for k in range(n_tan)], axis=2)
    assert int((info != 0).sum()) == 0
    r["max_rel_difference_exact_vs_central_differences"] = float(np.abs(H - fd).max() / np.abs(fd).max())
    r["max_rel_difference_along_tangents_vs_central_differences"] = float(np.abs(d2A_along.cpu().numpy() - fd).max() / np.abs(fd).max())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="profiles/expr_second_bench.json")
    a = ap.parse_args()
    doc = {"tool": "tools/bench_expr_second.py", "reps": a.reps,
           "statistic": "median wall time around a device synchronise after one warm-up call; the routes of one comparison alternate in every repetition",
           "baselines": "the value pass, the tangent pass, the call without the curvature term and the difference route are measured in the same process",
           "results": {}}
    for name, (text, values) in CASES.items():
        doc["results"][name] = measure_case(text, values, a.reps)
        print(json.dumps({name: doc["results"][name]}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
