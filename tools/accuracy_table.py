"""Ratio e / yardstick of every case of tests/test_gpu_accuracy.py on this GPU -> profiles/accuracy.json and a Markdown table.

e = max|A_gpu - T| / max|T| against the long-double truth of tests/accuracy_ref.py; yardstick = max(e_oracle_schur, e_cholesky_schur, 16 eps),
what float64 delivers on the same inputs.  The tests assert ratio <= 32.  Per case the largest ratio over its cells, families and M / no M.
Likewise the stratification tests (conditioning of M per family; coef 2^k, M 2^j) and, per group of quantities, the derived outputs of
tests/test_gpu_accuracy_derived.py against their own float64 yardsticks (accuracy_ref.derived_float64_errors).

    python tools/accuracy_table.py [--dumps DIR] [--out profiles/accuracy.json]

--dumps DIR: take the raw GPU results from DIR/accuracy_<group>.npz -- the name tests/accuracy_gpu.py's run_in_child gives them; written by
`python tests/accuracy_gpu.py accuracy <group> DIR/accuracy_<group>.npz` with the group's environment -- instead of running the plans here.
The derived outputs come from DIR/derived_default.npz (`python tests/accuracy_gpu.py derived default DIR/derived_default.npz`) and, for the
second load route of the fused plans, DIR/derived_blocked_loads.npz (the same with `blocked_loads` and HOMMX_FUSED_LOADS=0).

    python tools/accuracy_table.py --nonlinear [--out profiles/accuracy_nonlinear.json]

--nonlinear: the nonlinear family instead (tests/test_gpu_accuracy_nonlinear.py against the long-double truth of tests/nonlinear_truth.py):
every test of that file is run here as a function, and every comparison it makes -- case, quantity, e, the float64 yardstick, the bound and
the ratio e / (bound / 32) -- is written per group (iteration, tangent, history, load, state, magnitude, slot) with the group's worst ratio.

"second_derivatives": the ratio of d2A per (case, family, cell, load route) -- the largest over the cell's blocks, each block against its own
yardstick (accuracy_ref.block_rel).
"""

import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import accuracy_gpu as G  # noqa: E402
import accuracy_ref as R  # noqa: E402

DERIVED_GROUPS = {"tensor": ("A",), "fields": ("strain", "flux"), "statistics": ("mean_strain", "mean_flux", "energy", "max_flux"),
                  "regions": R.REGION_QUANTITIES, "dA, grad": ("dA", "grad"), "dA_dM, grad_M": ("dA_dM", "grad_M"),
                  "loads": tuple(q for q in R.LOAD_QUANTITIES if q != "load_chi"), "load correctors": ("load_chi",)}


NONLINEAR_GROUPS = {"iteration": ("test_fourth_round", "test_fixed_point", "test_laminate_against_mpmath"), "tangent": ("test_tangent", "test_asymmetry_of_a_law_without_a_potential"),
                    "history": ("test_history_over_three_load_steps", "test_tangent_at_frozen_history"),
                    "load": ("test_loads_beside_a_law", "test_loads_of_the_fused_plan_on_the_blocked_route"), "state": ("test_state_tail",),
                    "magnitude": ("test_magnitude",), "slot": ("test_slot_path_and_lds_path",)}


def nonlinear(out):
    """Runs the tests of tests/test_gpu_accuracy_nonlinear.py as functions, over their own parameters, and writes what they compared."""
    import time

    import nonlinear_truth as NT
    import test_gpu_accuracy_nonlinear as N

    class Tmp:
        def mktemp(self, name):
            return tempfile.mkdtemp(prefix=name)

    loads = G.run_nonlinear_group()
    params = {"test_fourth_round": NT.ITERATION_CASES, "test_fixed_point": NT.ITERATION_CASES, "test_laminate_against_mpmath": [()],
              "test_tangent": NT.TANGENT_CASES,
              "test_asymmetry_of_a_law_without_a_potential": [()], "test_history_over_three_load_steps": [(s,) for s in NT.HISTORY_SHAPES],
              "test_tangent_at_frozen_history": [(s,) for s in NT.HISTORY_TANGENT_SHAPES], "test_loads_beside_a_law": [(loads, s) for s in NT.LOAD_SHAPES],
              "test_loads_of_the_fused_plan_on_the_blocked_route": [(Tmp(),)], "test_state_tail": [(s,) for s in NT.STATE_CASES],
              "test_magnitude": [(s,) for s in NT.MAGNITUDE_SHAPES], "test_slot_path_and_lds_path": [(None,), (True,)]}
    groups, t0 = {}, time.perf_counter()
    for group, tests in NONLINEAR_GROUPS.items():
        first = len(N.Held.LOG)
        for name in tests:
            for a in params[name]:
                getattr(N, name)(*a)
        records = N.Held.LOG[first:]
        worst = max(records, key=lambda r: r["worst_ratio"])
        groups[group] = {"worst_ratio": worst["worst_ratio"], "worst_case": f"{worst['test']}: {worst['worst_at']}", "tests": records}
    with open(out, "w") as f:
        # three significant digits and one test per line: the record is a thousand comparisons
        doc = {"bound_factor": R.FACTOR, "floor_eps": R.FLOOR_EPS, "wall_time_s": round(time.perf_counter() - t0, 1), "groups": groups}
        text = json.dumps(json.loads(json.dumps(doc), parse_float=lambda v: float(f"{float(v):.3g}")), separators=(",", ":"))
        f.write(text.replace('{"test":', '\n{"test":') + "\n")
    print("| Group | worst ratio | at |\n|---|---|---|")
    for group, g in groups.items():
        print(f"| {group} | {g['worst_ratio']:.2f} | {g['worst_case']} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dumps")
    ap.add_argument("--nonlinear", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.nonlinear:
        return nonlinear(args.out or os.path.join(ROOT, "profiles", "accuracy_nonlinear.json"))
    args.out = args.out or os.path.join(ROOT, "profiles", "accuracy.json")

    def results(group, tmp):
        if args.dumps:
            with np.load(os.path.join(args.dumps, f"accuracy_{group}.npz")) as z:
                return {k: z[k] for k in z.files}
        return G.run_accuracy_group(group) if group == "default" else G.run_in_child("accuracy", group, tmp)

    with tempfile.TemporaryDirectory() as tmp:
        res = {g: results(g, tmp) for g in R.STRUCTURED_CASES}
    cache, rows = {}, []

    def ref(key, kind, x, cells, tp, coef, M, **kw):
        if key not in cache:
            T = R.truth(kind, x, cells, tp, coef, M)
            cache[key] = (T, R.float64_errors(kind, x, cells, tp, coef, M, T=T, **kw))
        return cache[key]

    def yard(e):
        return e["bound"] / R.FACTOR

    for group, cases in R.STRUCTURED_CASES.items():
        for kernel, kind, dim, n, flags in cases:
            x, cells, tp = R.structured(dim, n)
            worst = (0.0, 0.0, "")
            for family in R.FAMILIES[kind]:
                for wm in (False, True):
                    coef, M = R.structured_inputs(kind, dim, n, family, wm)
                    A = res[group][f"A|{G.skey(kind, dim, n, flags)}|{family}|{int(wm)}"]
                    for c in range(R.NC):
                        T, e = ref((kind, dim, n, family, wm, c), kind, x, cells, tp, coef[c], None if M is None else M[c], n=n)
                        err = R.rel(A[c], T[0])
                        worst = max(worst, (err / yard(e), err, f"{family}{' M' if wm else ''}"))
            rows.append({"group": group, "kernel": kernel, "case": f"{kind} {dim}D n={n}" + (" forced" if flags else ""), "ratio": worst[0],
                         "e": worst[1], "worst": worst[2]})
    for kernel, kind, builder, args_, route in R.MESH_CASES:
        worst = (0.0, 0.0, "")
        for family in R.FAMILIES[kind]:
            for wm in (False, True):
                msh, coef, M = R.mesh_inputs(kind, builder, args_, family, wm)
                x, cells, tp = R.mesh_arrays(msh)
                A = res["default"][f"A|{G.mkey(kind, builder, args_, route)}|{family}|{int(wm)}"]
                for c in range(R.NC):
                    T, e = ref((kind, builder, args_, family, wm, c), kind, x, cells, tp, coef[c], None if M is None else M[c], msh=msh)
                    err = R.rel(A[c], T[0])
                    worst = max(worst, (err / yard(e), err, f"{family}{' M' if wm else ''}"))
        rows.append({"group": "default", "kernel": kernel, "case": f"{kind} {builder}{args_}", "ratio": worst[0], "e": worst[1], "worst": worst[2]})
    for ckernel, kind, dim, n, group in R.CORRECTOR_CASES:
        x, cells, tp = R.structured(dim, n)
        worst = (0.0, 0.0, "")
        for family in R.FAMILIES[kind]:
            for wm in (False, True):
                coef, M = R.structured_inputs(kind, dim, n, family, wm)
                chi = res[group][f"corr|{G.skey(kind, dim, n, 0)}|{family}|{int(wm)}"]
                for c in range(R.NC):
                    T, e = ref((kind, dim, n, family, wm, c), kind, x, cells, tp, coef[c], None if M is None else M[c], n=n)
                    err = R.rel(chi[c].T, T[1])
                    worst = max(worst, (err / (e["bound_corr"] / R.FACTOR), err, f"{family}{' M' if wm else ''}"))
        rows.append({"group": group, "kernel": "correctors: " + ckernel, "case": f"{kind} {dim}D n={n}", "ratio": worst[0], "e": worst[1],
                     "worst": worst[2]})
    sweep = []
    for case in list(R.SWEEP_CASES) + [("default",) + R.SWEEP_MESH]:
        group = case[0]
        if isinstance(case[3], str):
            _, kernel, kind, builder, args_, route = case
            msh, coef, M = R.mesh_inputs(kind, builder, args_, "log2", True)
            x, cells, tp = R.mesh_arrays(msh)
            key, kw, ck, name = G.mkey(kind, builder, args_, route), {"msh": msh}, (kind, builder, args_, "log2", True), f"{kind} {builder}{args_}"
        else:
            _, kernel, kind, dim, n, flags = case
            coef, M = R.structured_inputs(kind, dim, n, "log2", True)
            x, cells, tp = R.structured(dim, n)
            key, kw, ck, name = G.skey(kind, dim, n, flags), {"n": n}, (kind, dim, n, "log2", True), f"{kind} {dim}D n={n}"
        per_k = {}
        for k in R.SWEEP_K:
            r = 0.0
            for c in range(R.NC):
                T, e = ref(ck + (c,), kind, x, cells, tp, coef[c], M[c], **kw)
                r = max(r, R.rel(res[group][f"sweepA|{key}|{k}"][c] * 2.0**-k, T[0]) / yard(e))
            per_k[str(k)] = r
        sweep.append({"group": group, "kernel": kernel, "case": name, "ratio_by_k": per_k})
    # the stratification on the tensor routes: conditioning (worst ratio per M family over two cells x log2 / top contrast) and scale
    m_cond, m_scale = [], []
    for case in R.M_CASES:
        group, case = case[0], case[1:]
        cid = R.case_id(case)
        per_family = {}
        for mf in R.M_CONDITIONING:
            worst = (0.0, 0.0, "")
            for family in ("log2", R.top_family(case[1])):
                coef, M, g = R.case_inputs(case, family, mf)
                for c in range(R.NC):
                    T, e = ref(("M", cid, family, mf, c), case[1], g["x"], g["cells"], g["tp"], coef[c], M[c], **g["kw"])
                    err = R.rel(res[group][f"MA|{cid}|{family}|{mf}"][c], T[0])
                    worst = max(worst, (err / yard(e), err, family))
            per_family[mf] = {"ratio": worst[0], "e": worst[1], "worst": worst[2]}
        m_cond.append({"group": group, "case": cid, "by_family": per_family})
        coef, M, g = R.case_inputs(case, "log2", "mild")
        per_kj = {}
        for k, j in R.M_SCALES:
            r = 0.0
            for c in range(R.NC):
                T, e = ref(("M", cid, "log2", "mild", c), case[1], g["x"], g["cells"], g["tp"], coef[c], M[c], **g["kw"])
                r = max(r, R.rel(res[group][f"MsA|{cid}|{k}|{j}"][c] * 2.0**-k, T[0]) / yard(e))
            per_kj[f"{k},{j}"] = r
        m_scale.append({"group": group, "case": cid, "ratio_by_kj": per_kj})
    # derived outputs: worst ratio e / float64 yardstick per case and group of quantities, over two cells x five families
    if args.dumps:
        with np.load(os.path.join(args.dumps, "derived_default.npz")) as z:
            dres = {k: z[k] for k in z.files}
    else:
        dres = G.run_derived_group()
    # the second load route of the fused plans (HOMMX_FUSED_LOADS=0: a child process)
    if args.dumps:
        with np.load(os.path.join(args.dumps, "derived_blocked_loads.npz")) as z:
            bres = {k: z[k] for k in z.files}
    else:
        with tempfile.TemporaryDirectory() as tmp:
            bres = G.run_in_child("derived", "blocked_loads", tmp)
    derived, second = [], []
    for case in R.DERIVED_CASES:
        kernel, ckernel, cs = R.derived_case(case)
        cid = R.case_id(cs)
        inp = R.derived_inputs(cs, R.case_inputs(cs, "log2", None)[0][0])
        worst = {name: (0.0, 0.0, "") for name in DERIVED_GROUPS}
        for fi, (family, mf) in enumerate(R.DERIVED_FAMILIES):
            coef, M, g = R.case_inputs(cs, family or R.top_family(cs[1]), mf)
            for c in range(R.NC):
                a = (cs[1], g["x"], g["cells"], g["tp"], coef[c], None if M is None else M[c])
                T = R.derived_truth(*a, **inp)
                y = R.derived_float64_errors(*a, **inp, T=T, **g["kw"])
                for gname, names in DERIVED_GROUPS.items():
                    for name in names:
                        key = f"d|{cid}|{fi}|{name}"
                        if key in dres:
                            v = dres[key][c]
                            err = R.rel(v.T if name == "load_chi" else v, T[name])
                            worst[gname] = max(worst[gname], (err / (y["bound"][name] / R.FACTOR), err, f"{name} {family or R.top_family(cs[1])} {mf or 'no M'}"))
                # d2A per block (accuracy_ref.block_rel), on every load route: the plan's own, and the blocked family's on the fused plans
                euler = R.euler_directions(coef[c], inp["directions"])
                for route, rr in ((("fused2d_subst" if kernel == "fused2d" else ckernel), dres), ("blocked", bres)):
                    key = f"d|{cid}|{fi}|d2A"
                    if key in rr:
                        err = R.block_rel(rr[key][c], T["d2A"], euler)
                        ratio = err / (y["bound"]["d2A"] / R.FACTOR)
                        at = np.unravel_index(ratio.argmax(), ratio.shape)
                        second.append({"case": cid, "family": family or R.top_family(cs[1]), "M": mf or "no M", "cell": c, "load_route": route,
                                       "ratio": float(ratio[at]), "e": float(err[at]), "e_float64": float(y["e"]["d2A"][at]), "block": [int(v) for v in at]})
        derived.append({"case": cid, "correctors": ckernel, "by_group": {k: {"ratio": v[0], "e": v[1], "worst": v[2]} for k, v in worst.items()}})
    with open(args.out, "w") as f:
        json.dump({"bound_factor": R.FACTOR, "floor_eps": R.FLOOR_EPS, "cases": rows, "magnitude_sweep": sweep, "stratification_conditioning": m_cond,
                   "stratification_scale": m_scale, "derived": derived, "second_derivatives": second}, f, indent=1)
    print("| Route | Case | worst ratio | e | at |\n|---|---|---|---|---|")
    for r in rows:
        print(f"| `{r['kernel']}`{'' if r['group'] == 'default' else ' (' + r['group'] + ')'} | {r['case']} | {r['ratio']:.2f} | {r['e']:.1e} | {r['worst']} |")
    print("\n| Route | Case | " + " | ".join(f"2^{k}" for k in R.SWEEP_K) + " |\n|---|---|" + "---|" * len(R.SWEEP_K))
    for s in sweep:
        print(f"| `{s['kernel']}` | {s['case']} | " + " | ".join(f"{s['ratio_by_k'][str(k)]:.2f}" for k in R.SWEEP_K) + " |")

    print("\nDerived outputs\n| Case | correctors | " + " | ".join(DERIVED_GROUPS) + " | worst at |\n|---|---|" + "---|" * (len(DERIVED_GROUPS) + 1))
    for d in derived:
        top = max(d["by_group"].values(), key=lambda v: v["ratio"])
        print(f"| {d['case']} | `{d['correctors']}` | " + " | ".join(f"{d['by_group'][k]['ratio']:.2f}" for k in DERIVED_GROUPS) + f" | {top['worst']} |")
    print("\nSecond derivatives: worst per-block ratio per case and load route\n| Case | load route | ratio | e | e_float64 | at |\n|---|---|---|---|---|---|")
    for cid, route in dict.fromkeys((s["case"], s["load_route"]) for s in second):
        w = max((s for s in second if (s["case"], s["load_route"]) == (cid, route)), key=lambda s: s["ratio"])
        print(f"| {cid} | `{route}` | {w['ratio']:.2f} | {w['e']:.1e} | {w['e_float64']:.1e} | {w['family']} {w['M']} cell {w['cell']} block {tuple(w['block'])} |")
    print("\nConditioning of M\n| Case | " + " | ".join(R.M_CONDITIONING) + " |\n|---|" + "---|" * len(R.M_CONDITIONING))
    for m in m_cond:
        print(f"| {m['case']}{'' if m['group'] == 'default' else ' (' + m['group'] + ')'} | "
              + " | ".join(f"{m['by_family'][f]['ratio']:.2f} ({m['by_family'][f]['worst']})" for f in R.M_CONDITIONING) + " |")
    print("\nScale of M: coef 2^k, M 2^j\n| Case | " + " | ".join(f"({k}, {j})" for k, j in R.M_SCALES) + " |\n|---|" + "---|" * len(R.M_SCALES))
    for m in m_scale:
        print(f"| {m['case']} | " + " | ".join(f"{m['ratio_by_kj'][f'{k},{j}']:.2f}" for k, j in R.M_SCALES) + " |")


if __name__ == "__main__":
    main()
