"""Cost of the load solve of the tree routes by substitution on the kept fronts (HOMMX_FLAG_TREE_LOADS) against one more
elimination with the load rows overridden, which is what every tree plan did before the flag and still does without it.

    python tools/bench_tree_loads.py [--parent-lib PATH/libhommx_hip.so] [--rounds 2] [--out profiles/tree_loads_bench.json]
    python tools/bench_tree_loads.py --case el16 --profile-leg second      # under rocprofv3 --kernel-trace --stats: the flagged plan alone

Cases: 256 cells of 16^3 3D elasticity ("multifrontal", C4 / C5 size) and 8,192 cells of 64^2 2D Poisson (plane block 64: the tree route).
Per case three device entries, every array resident on the device:
    response   hommx_loads_source_device: one load shared by all cells; energy and statistics, no fields
    secant     hommx_secant_load_source_device: ONE round (max_iter = 1) with a per-cell polarisation beside a softening law
    second     hommx_second_sensitivity_source_device: four shared directions (t loads per direction and cell)
Two builds: `base` -- the library named by --parent-lib (a build of the parent commit, loaded through HOMMX_LIB) or, without it, this
tree's library; in both the plan is created WITHOUT the flag -- and `subst`, this tree's library with the flag.  Every measurement
runs in a fresh process (the worker, --leg): one warm-up call per entry, then three timed calls, a device synchronise inside the clock.
The driver alternates the builds process by process, --rounds processes each, and reports per entry the median over each build's timed
calls and the medians of its processes."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (description, dim, n, kind, cells)
CASES = {"el16": ("16^3 3D elasticity", 3, 16, "elasticity", 256), "p64": ("64^2 2D Poisson", 2, 64, "poisson", 8192)}
ENTRIES = ("response", "secant", "second")
TIMED = 3


def entries(p, nc, rng):
    """{name: call} of the three device entries on plan `p`, the info tensor they write and what must stay alive."""
    import torch

    from hommx_amd import _lib
    from hommx_amd.expr import SecantLaw

    dev = torch.device("cuda", p.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    t, el = p.t, (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    soft = "(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"
    law = SecantLaw("c[0]*" + soft) if p.kind == "poisson" else SecantLaw(lam="c[0]", mu="c[1]*" + soft)
    coef = up(rng.uniform(0.5, 2.0, (nc,) + el))
    P, Pc, dirs = up(rng.standard_normal((1, p.n_el, t))), up(0.3 * rng.standard_normal((nc, p.n_el, t))), up(rng.standard_normal((4,) + el))
    xi, rows = up(rng.standard_normal((nc, t))), up(np.zeros((nc, 3)))
    P_eff, energy, stats, A, d2A = new(nc, 1, t), new(nc, 1, 1), new(nc, 1, t + 2), new(nc, t, t), new(nc, 4, 4, t, t)
    state, mean_flux = new(nc, 3), new(nc, t)
    info = torch.empty(nc, dtype=torch.int32, device=dev)
    src = _lib.CoefSource()
    src.form, src.coef = _lib.COEF_SAMPLED, coef.data_ptr()
    s = torch.cuda.current_stream(dev).cuda_stream
    keep = (coef, P, Pc, dirs, xi, rows, P_eff, energy, stats, A, d2A, state, mean_flux, law)
    return {
        "response": lambda: p.loads_device(nc, src, None, 1, P.data_ptr(), P_eff.data_ptr(), False, A.data_ptr(), info.data_ptr(), energy.data_ptr(),
                                           stats.data_ptr(), stream=s),
        "secant": lambda: p.secant_device(nc, src, None, xi.data_ptr(), law, rows.data_ptr(), state.data_ptr(), A.data_ptr(), max_iter=1,
                                          mean_flux_ptr=mean_flux.data_ptr(), info_ptr=info.data_ptr(), stream=s, P_ptr=Pc.data_ptr()),
        "second": lambda: p.second_sensitivities_device(nc, src, None, 4, dirs.data_ptr(), d2A.data_ptr(), False, None, A.data_ptr(), info.data_ptr(),
                                                        stream=s),
    }, info, keep


def leg(case, flagged, reps, only=None):
    """The worker: one plan in this process, every entry (or `only`) warmed once and timed `reps` times; one JSON line."""
    import torch

    from hommx_amd import MicroCellPlan, _lib

    name, dim, n, kind, nc = CASES[case]
    p = MicroCellPlan(dim, n, kind, **({"tree_loads": True} if flagged else {}))
    assert p.kernel == "multifrontal" and p.load_kernel == ("multifrontal_subst" if flagged else "multifrontal"), (p.kernel, p.load_kernel)
    calls, info, keep = entries(p, nc, np.random.default_rng(0))
    out = {"case": case, "flagged": flagged, "lib": _lib.LIB_PATH, "load_kernel": p.load_kernel}
    for entry in ENTRIES if only is None else (only,):
        ts = []
        for rep in range(reps + 1):  # the first call is the warm-up: it allocates the arena
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[entry]()
            torch.cuda.synchronize()
            if rep:
                ts.append(time.perf_counter() - t0)
        assert int((info != 0).sum()) == 0
        out[entry] = ts
    print("LEG " + json.dumps(out), flush=True)


def run_leg(case, flagged, lib):
    env = dict(os.environ)
    env.pop("HOMMX_LIB", None)
    if lib:
        env["HOMMX_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", case] + (["--flagged"] if flagged else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode:
        raise RuntimeError(f"worker failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(next(line for line in r.stdout.splitlines() if line.startswith("LEG "))[4:])


def measure(parent_lib, rounds, only):
    out = []
    for case, (name, dim, n, kind, nc) in CASES.items():
        if only and only != case:
            continue
        legs = {"base": [], "subst": []}
        for _ in range(rounds):  # base, subst, base, subst, ...: each a fresh process
            legs["base"].append(run_leg(case, False, parent_lib))
            legs["subst"].append(run_leg(case, True, None))
        r = {"case": name, "cells": nc, "base_library": "parent commit" if parent_lib else "this tree, plan without the flag"}
        for entry in ENTRIES:
            for which in legs:
                pooled = [t for l in legs[which] for t in l[entry]]
                r[f"{entry}_{which}_s"] = float(np.median(pooled))
                r[f"{entry}_{which}_process_medians_s"] = [float(np.median(l[entry])) for l in legs[which]]
            r[f"{entry}_speedup"] = r[f"{entry}_base_s"] / r[f"{entry}_subst_s"]
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libhommx_hip.so built from the parent commit: the `base` build")
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per build and case")
    ap.add_argument("--out", default="profiles/tree_loads_bench.json")
    ap.add_argument("--case", choices=tuple(CASES), default=None)
    ap.add_argument("--leg", choices=tuple(CASES), default=None, help="worker: one plan in this process")
    ap.add_argument("--flagged", action="store_true")
    ap.add_argument("--profile-leg", choices=ENTRIES, default=None, help="one entry of the flagged plan of --case alone, for a kernel trace")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.flagged, TIMED)
    if a.profile_leg:
        return leg(a.case or "el16", True, TIMED, a.profile_leg)
    doc = {"tool": "tools/bench_tree_loads.py", "timed_calls_per_process": TIMED, "processes_per_build": a.rounds,
           "statistic": "median wall time over the timed calls of a build's processes; one warm-up call per entry and process; the builds alternate "
                        "process by process; device entries, arrays resident, a device synchronise inside the clock",
           "results": measure(os.path.abspath(a.parent_lib) if a.parent_lib else None, a.rounds, a.case)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
