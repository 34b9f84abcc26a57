"""What an expression coefficient costs: the headline batch -- 8,192 macro cells of 32^2 micro cells, scalar
Poisson -- with five coefficients:

    two_phase    TwoPhase, |y0 - 1/2| < 1/4 ? 5 + 2 x0 : 1            the fused kernel selects in registers
    where        the same medium as Expression("where(...)")            degree 0: bytecode kernel, 1 point per element, STREAM mode
    separable    Separable affine, 1.1 + x0 + sin(2 pi y0)              the fused kernel forms a + b g in registers
    expression   the same coefficient as an Expression                  degree 3: bytecode kernel, 6 points per element, STREAM mode
    callable     the same coefficient as a Python callable, degree 3    sampled with NumPy on the host, the means cross the bus

    python tools/bench_expr.py [--reps 5] [--out profiles/expr_bench.json]

Per coefficient, median (min, max) wall time over the repetitions after one warm-up of: `stream_s`, forming the CoefStream on the host
(the callable: 10^8 evaluations; the others: a mask, a table or the quadrature points); `plan_s`, the plan-level host call on that
stream (inputs in, A_eff out, synchronised); `device_s`, the device entry on inputs already resident (kernels alone); `solve_s`,
PoissonHMM.solve() end to end with a forced re-assembly (stream + plan call + macro assembly and solve)."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NX, N = 64, 32


def coefficients():
    from hommx_amd import hmm

    smooth = "1.1 + x[0] + sin(2*pi*y[0])"
    return {
        "two_phase": (hmm.TwoPhase(lambda y: np.abs(y[0] - 0.5) < 0.25, lambda x: 5 + 2 * x[0], lambda x: 1.0 + 0.0 * x[0]), None),
        "where": (hmm.Expression("where(abs(y[0] - 0.5) < 0.25, 5 + 2*x[0], 1)"), None),
        "separable": (hmm.Separable("affine", lambda x: 1.1 + x[0], lambda x: 1.0 + 0.0 * x[0], lambda y: np.sin(2 * np.pi * y[0])), None),
        "expression": (hmm.Expression(smooth), None),
        "callable": (lambda x, y: 1.1 + x[0] + np.sin(2 * np.pi * y[0]), 3),
    }


def timed(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def measure(reps):
    import torch

    from hommx_amd import hmm, mesh

    msh, micro = mesh.create_unit_square(NX, NX), mesh.create_unit_square(N, N)
    cells = np.arange(msh.num_cells)
    out = {"cells": int(msh.num_cells), "n_micro": N, "reps": reps, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, (A, degree) in coefficients().items():
        h = hmm.PoissonHMM(msh, A, lambda x: 1.0 + x[0], micro, 1.0 / 128, quadrature_degree=degree)
        stream, kind = h._coef_stream(cells)
        plan = h._ensure_plan(kind)
        dev = torch.device("cuda", plan.device)
        sync = lambda: torch.cuda.synchronize(dev)
        r = {"form": stream.method, "kernel": plan.kernel, "quadrature_degree": h.quadrature_degree_used,
             "bytes_per_cell_in": float(stream.per_cell.nbytes / len(cells))}
        r["stream_s"] = timed(lambda: h._coef_stream(cells), reps, sync)
        A_host, info = stream.solve(plan, None, return_info=True)
        assert not info.any()
        r["plan_s"] = timed(lambda: stream.solve(plan, None, return_info=True), reps, sync)
        keep = []

        def upload(a):
            keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
            return keep[-1].data_ptr()

        src = stream.coef_source(upload)
        A_dev = torch.empty((len(cells), 2, 2), dtype=torch.float64, device=dev)
        i_dev = torch.empty((len(cells),), dtype=torch.int32, device=dev)
        run = lambda: plan.solve_source_device(len(cells), src, None, A_dev.data_ptr(), i_dev.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        r["device_s"] = timed(run, reps, sync)
        assert np.array_equal(A_dev.cpu().numpy(), A_host)

        def solve():
            h._needs_reassembly = True
            h.solve()

        r["solve_s"] = timed(solve, reps, sync)
        r["solves_per_s_plan"] = len(cells) / r["plan_s"]["median"]
        r["solves_per_s_device"] = len(cells) / r["device_s"]["median"]
        out["cases"][name] = r
        print(f"{name:11s} stream {r['stream_s']['median'] * 1e3:9.2f} ms  plan {r['plan_s']['median'] * 1e3:8.2f} ms  device "
              f"{r['device_s']['median'] * 1e3:8.2f} ms  PoissonHMM.solve {r['solve_s']['median'] * 1e3:9.2f} ms", flush=True)
    c = out["cases"]
    # the interpreted pass and the stream's round trip through HBM: the program form against the sampled stream it expands to
    out["expression_over_separable_device"] = c["expression"]["device_s"]["median"] / c["separable"]["device_s"]["median"]
    out["where_over_two_phase_device"] = c["where"]["device_s"]["median"] / c["two_phase"]["device_s"]["median"]
    out["callable_over_expression_solve"] = c["callable"]["solve_s"]["median"] / c["expression"]["solve_s"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "expr_bench.json"))
    args = ap.parse_args()
    res = measure(args.reps)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "cases"}))


if __name__ == "__main__":
    main()
