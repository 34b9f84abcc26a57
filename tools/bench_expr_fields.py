"""Cost of the per-cell fields f[k] of an expression coefficient (hommx_coef_source.n_fields) on the headline batch:
8,192 cells of 32^2 scalar Poisson at degree 3, A = 1.1 + x[0] + a sin(2 pi y[0]) + b cos(2 pi y[1]).

    python tools/bench_expr_fields.py --parent <checkout of the parent commit, its library built> [--rounds 3] [--reps 7]
                                      [--out profiles/expr_fields_bench.json]

(1) What the row stride costs a program WITHOUT fields: the value pass (expand_device) and the two-slot tangent pass
    (expand_tangents_device) of the p-only program (a = p[0], b = p[1]) on this tree against the parent commit's, on the same box in the
    same session -- each tree in a fresh child process (``--leg passes --tree DIR``), the two alternating ``--rounds`` times.  A pass is
    timed as a window of ``LAUNCHES`` launches closed by one synchronise, the statistic is the median of ``--reps`` windows, and a tree's
    figure is the median over its rounds.  The spread of the parent's own rounds is recorded beside the ratio.  Gate: no more than 3 %
    slower (the box-to-box spread the README states).
(2) Recorded without a gate: the same program with its amplitude a field (a = f[0], one value per cell; b = p[0]) -- the on-demand load
    of the row -- and ``PoissonHMM.tensor_derivatives()`` with one field against the same direction as a Python callable.
Without ``--parent`` only this tree is measured and (1) has no ratio."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_P, P = "1.1 + x[0] + p[0]*sin(2*pi*y[0]) + p[1]*cos(2*pi*y[1])", [0.5, 0.25]
TEXT_F, P_F, F_VALUE = "1.1 + x[0] + f[0]*sin(2*pi*y[0]) + p[0]*cos(2*pi*y[1])", [0.25], 0.5
TEXT_HMM = "1.1 + x[0] + f[0]*sin(2*pi*y[0]) + 0.25*cos(2*pi*y[1])"
N_MACRO, N_MICRO = 64, 32  # 2 * 64^2 = 8,192 macro cells
LAUNCHES = 40  # per timed window: 0.1 s of the value pass, 0.27 s of the tangent pass


def window_time(fn, reps, launches=LAUNCHES):
    """Median over ``reps`` windows of the time of one call: ``launches`` calls, one synchronise."""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / launches)
    return float(np.median(ts))


def passes(A, rows, reps, **counts):
    """Value pass and tangent pass of expression A on the headline batch, everything resident (the API both trees have)."""
    import torch

    from hommx_amd import MicroCellPlan, hmm, mesh as Mm
    from hommx_amd.batch import CoefStream

    micro = Mm.create_unit_square(N_MICRO, N_MICRO)
    bary, w = hmm.micro_quadrature(2, A.degree)
    yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, micro.cell_vertices()))
    p = MicroCellPlan(2, N_MICRO, "poisson")
    stream = CoefStream.program(yq, w, *A.program(), A.n_comp, rows, **counts)
    nc, n_tan = len(rows), sum(counts.values())
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    src = stream.coef_source(upload)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_coef = torch.empty((nc, p.n_el), dtype=torch.float64, device=dev)
    d_dirs = torch.empty((nc, n_tan, p.n_el), dtype=torch.float64, device=dev)
    r = {"value_pass_s": window_time(lambda: p.expand_device(nc, src, d_coef.data_ptr(), s), reps),
         "tangent_pass_s": window_time(lambda: p.expand_tangents_device(nc, src, d_coef.data_ptr(), d_dirs.data_ptr(), s), reps)}
    r["checksum"] = [float(d_coef.sum().item()), float(d_dirs.sum().item())]  # the two trees must compute the same
    return r, {"cells": nc, "n_micro": N_MICRO, "degree": A.degree, "n_q": int(len(w)), "n_ops": int(A.program()[0].shape[0]), "slots": n_tan}


def leg_passes(tree, reps):
    """Child process: the p-only program on the package of ``tree``."""
    sys.path.insert(0, tree)
    from hommx_amd import hmm, mesh as Mm

    rows = Mm.create_unit_square(N_MACRO, N_MACRO).cell_midpoints()
    r, _ = passes(hmm.Expression(TEXT_P, p=P), rows, reps, n_params=2)
    print("RESULT " + json.dumps(r), flush=True)


def child(tree, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "passes", "--tree", tree, "--reps", str(reps)], check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return json.loads([line for line in out.splitlines() if line.startswith("RESULT ")][-1][7:])


def measure(parent, rounds, reps):
    r = {"expression_without_fields": TEXT_P, "p": P, "launches_per_window": LAUNCHES}
    # (1) this tree against the parent, alternating
    runs = {"parent": [], "this": []}
    for _ in range(rounds):
        if parent:
            runs["parent"].append(child(os.path.abspath(parent), reps))
        runs["this"].append(child(HERE, reps))
    for key in ("value_pass_s", "tangent_pass_s"):
        for tree, got in runs.items():
            if got:
                ts = [g[key] for g in got]
                r[f"{tree}_{key}"] = float(np.median(ts))
                r[f"{tree}_{key}_rounds"] = ts
        if parent:
            r[key.replace("_s", "_this_over_parent")] = r[f"this_{key}"] / r[f"parent_{key}"]
    if parent:
        r["same_checksums"] = all(g["checksum"] == runs["this"][0]["checksum"] for got in runs.values() for g in got)
        r["within_3_percent"] = bool(r["value_pass_this_over_parent"] <= 1.03 and r["tangent_pass_this_over_parent"] <= 1.03)
    print(json.dumps(r, indent=1), flush=True)
    # (2) the amplitude as a field, in this process
    sys.path.insert(0, HERE)
    from hommx_amd import hmm, mesh as Mm

    msh, micro = Mm.create_unit_square(N_MACRO, N_MACRO), Mm.create_unit_square(N_MICRO, N_MICRO)
    x = msh.cell_midpoints()
    rows = np.ascontiguousarray(np.concatenate([x, np.full((len(x), 1), F_VALUE)], axis=1))
    f, shape = passes(hmm.Expression(TEXT_F, p=P_F, fields=1), rows, reps, n_params=1, n_fields=1)
    r.update(shape)
    r.update({"expression_with_a_field": TEXT_F, "field_value_pass_s": f["value_pass_s"], "field_tangent_pass_s": f["tangent_pass_s"],
              "field_value_pass_over_p_only": f["value_pass_s"] / r["this_value_pass_s"],
              "field_tangent_pass_over_p_only": f["tangent_pass_s"] / r["this_tangent_pass_s"]})
    h = hmm.PoissonHMM(msh, hmm.Expression(TEXT_HMM, fields=1), lambda x: 1.0 + x[0], micro, 0.01)
    h.set_fields(0.25 + 0.5 * x[:, 0] * x[:, 1])
    direction = [lambda x, y: np.sin(2 * np.pi * y[0]) + 0.0 * x[0]]
    a, b = h.tensor_derivatives(), h.tensor_derivatives(directions=direction)
    r["hmm_expression"] = TEXT_HMM
    r["hmm_max_rel_difference_of_dA"] = float(np.abs(a.dA - b.dA).max() / np.abs(b.dA).max())
    r["hmm_tensor_derivatives_field_s"] = window_time(lambda: h.tensor_derivatives(), reps, 1)
    r["hmm_tensor_derivatives_callable_s"] = window_time(lambda: h.tensor_derivatives(directions=direction), min(reps, 3), 1)
    r["hmm_speedup_over_callable"] = r["hmm_tensor_derivatives_callable_s"] / r["hmm_tensor_derivatives_field_s"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with hommx_amd/libhommx_hip.so built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/expr_fields_bench.json")
    ap.add_argument("--leg", default=None)
    ap.add_argument("--tree", default=HERE)
    a = ap.parse_args()
    if a.leg == "passes":
        return leg_passes(a.tree, a.reps)
    doc = {"tool": "tools/bench_expr_fields.py", "rounds": a.rounds, "reps": a.reps,
           "statistic": f"median of {a.reps} windows of {LAUNCHES} launches and one synchronise each; per tree, the median over its rounds",
           "baseline": "the parent commit, built from a checkout of it, measured in the same session in alternation with this tree",
           "results": measure(a.parent, a.rounds, a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
