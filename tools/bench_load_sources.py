"""What it costs to bring a polarisation load to the device (hommx_loads_source): ready-made per-cell element means
against the program of a vector ``Expression`` (HOMMX_LOADS_PROGRAM) against an eigenstrain program (HOMMX_LOADS_EIGENSTRAIN), on the
headline batch (8,192 cells of 32^2 scalar Poisson, the TwoPhase inclusion) and on 256 cells of 16^3 isotropic elasticity (the TwoPhase
fibre); and ``PoissonHMM.solve()`` on the headline batch with the load as a Python callable -- the only form it took before, sampled
on the host -- against the same load as an ``Expression``, as a polarisation and as an eigenstrain.

    python tools/bench_load_sources.py [--reps 5] [--out profiles/load_sources_bench.json]

Per case, the median wall time after one warm-up call.  ``loads``: the host entry, P_eff only, one load -- the per-cell array is
[N, 1, n_el, t] doubles that exist already (its sampling is not in the figure), the programs are sampled at the points of the degree-2
rule.  ``solve``: end to end with a forced re-assembly and the coefficient a ``TwoPhase`` (its rule, the centroid rule, samples the load
too); ``sample_s`` is the part of it that forms what crosses the boundary (``_polarisation_loads``)."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NX, N = 64, 32
ALPHA = "0.01*(1.0 + 0.5*sin(2*pi*y[0]))"


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


def strain(dim, t):
    """A thermal eigenstrain alpha(y) dT, dT the field of the macro cell: isotropic, no shear."""
    from hommx_amd import hmm

    return hmm.Expression([f"{ALPHA}*f[0]" if c < dim else "0.0*y[0]" for c in range(t)], fields=("dT",))


def plan_level(reps):
    import torch

    from hommx_amd import MicroCellPlan, hmm, mesh, workloads as W
    from hommx_amd.batch import CoefStream

    _, mask2, values2 = W.c2_inclusion_two_phase()
    _, mask4, values4, _ = W.c4_two_phase(cells=np.arange(256))
    out = []
    for name, dim, n, kind, mask, values in (("8192 cells, 32^2 Poisson", 2, 32, "poisson", mask2, values2),
                                             ("256 cells, 16^3 elasticity", 3, 16, "elasticity", mask4, values4)):
        p = MicroCellPlan(dim, n, kind)
        sync = lambda: torch.cuda.synchronize(torch.device("cuda", p.device))
        nc, t = values.shape[0], p.t
        coef = CoefStream.two_phase(mask, values)
        micro = mesh.create_unit_square(n, n) if dim == 2 else mesh.create_unit_cube(n, n, n)
        bary, w = hmm.micro_quadrature(dim, 2)
        yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, micro.cell_vertices()))
        rng = np.random.default_rng(0)
        rows = np.ascontiguousarray(np.concatenate([rng.uniform(0.0, 1.0, (nc, 3)), rng.uniform(0.5, 1.5, (nc, 1))], axis=1))
        E = strain(dim, t)
        load = CoefStream.program(yq, w, *E.program(), E.n_comp, rows, n_params=E.n_params, n_fields=E.n_fields)
        by_program = p.loads(coef, load, eigenstrain=True)
        assert not by_program.info.any()
        array = np.ascontiguousarray(np.broadcast_to(E.host_stream(rows[:1], yq, w)[0], (nc, 1, p.n_el, t)))  # ready-made element means
        r = {"case": name, "cells": nc, "n_el": p.n_el, "t": t, "kernel": p.kernel, "program_points": int(yq.shape[1]),
             "bytes_per_cell_array": float(array.nbytes / nc), "bytes_per_cell_program": float(rows.nbytes / nc)}
        r["loads_per_cell_array_s"] = timed(lambda: p.loads(coef, array, per_cell=True), reps, sync)
        r["loads_eigenstrain_array_s"] = timed(lambda: p.loads(coef, array, per_cell=True, eigenstrain=True), reps, sync)
        r["loads_program_s"] = timed(lambda: p.loads(coef, load), reps, sync)
        r["loads_eigenstrain_program_s"] = timed(lambda: p.loads(coef, load, eigenstrain=True), reps, sync)
        r["array_over_program"] = r["loads_per_cell_array_s"]["median"] / r["loads_program_s"]["median"]
        out.append(r)
        print(", ".join(f"{k} {v['median'] * 1e3:.2f} ms" if k.endswith("_s") else f"{k}: {v}" for k, v in r.items()), flush=True)
        del p
    return out


def solver_level(reps):
    import torch

    from hommx_amd import hmm, mesh, workloads as W

    msh, micro = mesh.create_unit_square(NX, NX), mesh.create_unit_square(N, N)
    dT = lambda x: 1.0 + 0.5 * x[0] - 0.25 * x[1]
    alpha = lambda y: 0.01 * (1.0 + 0.5 * np.sin(2 * np.pi * y[0]))
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 5.0 + 2.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
    E = strain(2, 2)
    forms = {
        "callable": lambda h: h.set_polarisation(lambda x, y: [-(tp(x, y) * (alpha(y) * dT(x)))] * 2),  # the eigenstress written by hand
        "expression_polarisation": lambda h: (h.set_polarisation(E), h.set_polarisation_fields(dT(msh.cell_midpoints().T))),
        "expression_eigenstrain": lambda h: (h.set_eigenstrain(E), h.set_polarisation_fields(dT(msh.cell_midpoints().T))),
        "none": lambda h: None,
    }
    out = {"cells": int(msh.num_cells), "n_micro": N, "coefficient": "TwoPhase", "cases": {}}
    cells = np.arange(msh.num_cells)
    for name, set_load in forms.items():
        h = hmm.PoissonHMM(msh, tp, lambda x: 1.0 + x[0], micro, 1.0 / 128)
        set_load(h)
        sync = lambda: torch.cuda.synchronize()

        def solve():
            h._needs_reassembly = True
            h.solve()

        r = {"solve_s": timed(solve, reps, sync)}
        if name != "none":
            kind = h._micro_kind()
            r["sample_s"] = timed(lambda: h._polarisation_loads(cells, kind), reps, sync)
            r["P_eff_max"] = float(np.abs(h.effective_polarisation).max())
        out["cases"][name] = r
        print(f"{name:24s} PoissonHMM.solve {r['solve_s']['median'] * 1e3:9.2f} ms" + (
            f"  of it forming the load {r['sample_s']['median'] * 1e3:9.2f} ms" if "sample_s" in r else ""), flush=True)
    c = out["cases"]
    out["callable_over_expression_solve"] = c["callable"]["solve_s"]["median"] / c["expression_eigenstrain"]["solve_s"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "load_sources_bench.json"))
    a = ap.parse_args()
    import torch

    doc = {"tool": "tools/bench_load_sources.py", "reps": a.reps, "statistic": "median wall time after one warm-up call",
           "device": torch.cuda.get_device_name(0), "loads": plan_level(a.reps), "solve": solver_level(a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"callable_over_expression_solve": doc["solve"]["callable_over_expression_solve"],
                      "array_over_program": [r["array_over_program"] for r in doc["loads"]]}))


if __name__ == "__main__":
    main()
