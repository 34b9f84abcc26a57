"""GPU side of the accuracy and pivot-contract tests: runs the case groups of tests/accuracy_ref.py through the plans and returns raw
results.  Nothing here computes a bound.  Environment knobs are read when a plan is created, so the forced groups run this module as a
child process:  python accuracy_gpu.py <accuracy|pivot|derived|nonlinear> <group> <out.npz>  (the derived outputs: the default group, and blocked_loads for the second load route of the fused plans; nonlinear: the load cases of tests/nonlinear_truth.py, the same two groups)."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

import accuracy_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def skey(kind, dim, n, flags):
    return f"{kind}_{dim}_{n}_{flags}"


def mkey(kind, builder, args, route):
    return f"{kind}_{builder}_{'x'.join(map(str, args))}_{route}"


def _plan(kernel, kind, dim, n, flags):
    from hommx_amd import MicroCellPlan

    p = MicroCellPlan(dim, n, kind, flags=flags)
    assert p.kernel == kernel, (p.kernel, kernel, kind, dim, n, flags)
    return p


def _mesh_plan(kernel, kind, msh, route):
    from hommx_amd import MicroCellPlan

    p = MicroCellPlan.from_mesh(msh, kind, route=route)
    assert p.kernel == kernel, (p.kernel, kernel)
    return p


def _families(kind):
    return [(f, m) for f in R.FAMILIES[kind] for m in (False, True)]


def run_accuracy_group(group: str) -> dict:
    """Every structured case of the group (and, in the default group, the mesh and corrector cases), every family with and without M, and
    the magnitude sweep of the group's kernel families."""
    out = {}
    for kernel, kind, dim, n, flags in R.STRUCTURED_CASES[group]:
        p = _plan(kernel, kind, dim, n, flags)
        for family, with_M in _families(kind):
            coef, M = R.structured_inputs(kind, dim, n, family, with_M)
            A, info = p.solve(coef, M, return_info=True)
            out[f"A|{skey(kind, dim, n, flags)}|{family}|{int(with_M)}"] = A
            out[f"info|{skey(kind, dim, n, flags)}|{family}|{int(with_M)}"] = info
    for g, kernel, kind, dim, n, flags in R.SWEEP_CASES:
        if g != group:
            continue
        p = _plan(kernel, kind, dim, n, flags)
        coef, M = R.structured_inputs(kind, dim, n, "log2", True)
        for k in R.SWEEP_K:
            A, info = p.solve(coef * 2.0**k, M, return_info=True)
            out[f"sweepA|{skey(kind, dim, n, flags)}|{k}"] = A
            out[f"sweepinfo|{skey(kind, dim, n, flags)}|{k}"] = info
    _run_stratification(group, out)
    if group != "default":
        return out
    for kernel, kind, builder, args, route in R.MESH_CASES:
        for family, with_M in _families(kind):
            msh, coef, M = R.mesh_inputs(kind, builder, args, family, with_M)
            p = _mesh_plan(kernel, kind, msh, route)
            A, info = p.solve(coef, M, return_info=True)
            out[f"A|{mkey(kind, builder, args, route)}|{family}|{int(with_M)}"] = A
            out[f"info|{mkey(kind, builder, args, route)}|{family}|{int(with_M)}"] = info
    kernel, kind, builder, args, route = R.SWEEP_MESH
    msh, coef, M = R.mesh_inputs(kind, builder, args, "log2", True)
    p = _mesh_plan(kernel, kind, msh, route)
    for k in R.SWEEP_K:
        A, info = p.solve(coef * 2.0**k, M, return_info=True)
        out[f"sweepA|{mkey(kind, builder, args, route)}|{k}"] = A
        out[f"sweepinfo|{mkey(kind, builder, args, route)}|{k}"] = info
    for ckernel, kind, dim, n, _ in R.CORRECTOR_CASES:
        from hommx_amd import MicroCellPlan

        p = MicroCellPlan(dim, n, kind)
        assert p.corrector_kernel == ckernel, (p.corrector_kernel, ckernel)
        for family, with_M in _families(kind):
            coef, M = R.structured_inputs(kind, dim, n, family, with_M)
            A, chi, info = p.solve(coef, M, return_info=True, return_correctors=True)
            out[f"corrA|{skey(kind, dim, n, 0)}|{family}|{int(with_M)}"] = A
            out[f"corr|{skey(kind, dim, n, 0)}|{family}|{int(with_M)}"] = chi
            out[f"corrinfo|{skey(kind, dim, n, 0)}|{family}|{int(with_M)}"] = info
    # correctors and user-supplied loads with coefficient AND loads scaled by 2^k
    for kind, dim, n in R.SWEEP_LOAD_CASES:
        from hommx_amd import MicroCellPlan

        p = MicroCellPlan(dim, n, kind)
        coef, M = R.structured_inputs(kind, dim, n, "log2", True)
        P = R.load_inputs(kind, dim, n)
        for k in R.SWEEP_LOAD_K:
            A, chi, info = p.solve(coef * 2.0**k, M, return_info=True, return_correctors=True)
            r = p.loads(coef * 2.0**k, P * 2.0**k, M, response=True, return_correctors=True)
            tail = f"{skey(kind, dim, n, 0)}|{k}"
            out["lsw_chi|" + tail], out["lsw_info|" + tail] = chi, np.maximum(info, r.info)
            out["lsw_Peff|" + tail], out["lsw_energy|" + tail], out["lsw_mean|" + tail] = r.P_eff, r.energy, r.mean_flux
            out["lsw_lchi|" + tail] = r.correctors
    return out


def _case_plan(case, geometry):
    """The plan of a case without its group, structured or mesh, with its route asserted."""
    if R.is_mesh_case(case):
        return _mesh_plan(case[0], case[1], geometry["kw"]["msh"], case[4])
    return _plan(*case[:4], case[4] if len(case) > 4 else 0)


def _run_stratification(group: str, out: dict):
    """The M_CASES of the group: badly conditioned M on log2 and the top-contrast family, and log2 with coef * 2^k, M * 2^j."""
    for case in R.M_CASES:
        if case[0] != group:
            continue
        case, cid = case[1:], R.case_id(case[1:])
        p = None
        for family in ("log2", R.top_family(case[1])):
            for mf in R.M_CONDITIONING:
                coef, M, g = R.case_inputs(case, family, mf)
                p = p or _case_plan(case, g)
                out[f"MA|{cid}|{family}|{mf}"], out[f"Minfo|{cid}|{family}|{mf}"] = p.solve(coef, M, return_info=True)
        coef, M, _ = R.case_inputs(case, "log2", "mild")
        for k, j in R.M_SCALES:
            out[f"MsA|{cid}|{k}|{j}"], out[f"Msinfo|{cid}|{k}|{j}"] = p.solve(coef * 2.0**k, M * 2.0**j, return_info=True)


def _derived_calls(p, coef, M, inp, with_response: bool) -> dict:
    """One call each of reconstruct, sensitivities, stratification_sensitivities and loads on NC cells; the arrays under the names of
    accuracy_ref.derived_truth, ``info`` the largest of the four."""
    nc = coef.shape[0]
    tile = lambda v: np.ascontiguousarray(np.broadcast_to(v, (nc,) + v.shape))  # noqa: E731
    r = p.reconstruct(coef, tile(inp["xi"]), M, fields=True, regions=inp["labels"])
    s = p.sensitivities(coef, M, directions=inp["directions"], weights=tile(inp["weights"]))
    m = p.stratification_sensitivities(coef, M, weights=tile(inp["weights"]), full=True)
    out = {"A": r.A_eff, "strain": r.strain, "flux": r.flux, "mean_strain": r.mean_strain, "mean_flux": r.mean_flux, "energy": r.energy,
           "max_flux": r.max_flux, "argmax": r.argmax_element, "region_volume": r.region_volume, "region_mean_strain": r.region_mean_strain,
           "region_mean_flux": r.region_mean_flux, "region_energy": r.region_energy, "region_max_flux": r.region_max_flux,
           "region_argmax": r.region_argmax_element, "dA": s.dA, "grad": s.grad, "dA_dM": m.dA_dM, "grad_M": m.grad_M}
    info = np.maximum(np.maximum(r.info, s.info), m.info)
    if with_response:
        out.update(_load_calls(p, coef, M, inp, s.dA))
    else:  # the frontal mesh route solves no load problem: P_eff by Levin's identity alone, and no second derivatives
        l = p.loads(coef, inp["loads"], M)
        out.update(P_eff=l.P_eff, info=l.info)
    out["info"] = np.maximum(info, out["info"])
    return out


def _load_calls(p, coef, M, inp, dA=None) -> dict:
    """The two calls that solve load problems, loads and second_sensitivities, on a plan with a load solve; ``info`` the larger of the two.
    The first derivatives of second_sensitivities are the bits of ``dA`` (those of sensitivities() on the same inputs)."""
    l = p.loads(coef, inp["loads"], M, response=True, fields=True, return_correctors=True)
    s2 = p.second_sensitivities(coef, M, directions=inp["directions"], first=True)
    assert np.array_equal(s2.dA, p.sensitivities(coef, M, directions=inp["directions"]).dA if dA is None else dA)
    return dict(load_chi=l.correctors, P_eff=l.P_eff, load_mean_flux=l.mean_flux, load_energy=l.energy, load_strain=l.strain, load_flux=l.flux,
                load_max_flux=l.max_flux, load_argmax=l.argmax_element, d2A=s2.d2A, info=np.maximum(l.info, s2.info))


def run_derived_group(group: str = "default") -> dict:
    """Every derived output of every DERIVED_CASES case and family (keys d|case|family index|name), and of the DERIVED_SWEEP_CASES with
    coef * 2^k, M * 2^j, loads * 2^k (keys dsw|case|k|j|name) and with directions * 2^i alone (keys ddir|case|i|name: dA, d2A, info).

    group 'blocked_loads' (a child process with HOMMX_FUSED_LOADS=0): the fused cases alone, and of them the calls that solve load problems
    (loads, second_sensitivities), with the load route asserted; the same keys d|case|family index|name."""
    out = {}
    for case in R.DERIVED_CASES:
        kernel, ckernel, cs = R.derived_case(case)
        if group == "blocked_loads" and kernel != "fused2d":
            continue
        cid = R.case_id(cs)
        coef0, _, g = R.case_inputs(cs, "log2", None)
        inp = R.derived_inputs(cs, coef0[0])
        p = _case_plan(cs, g)
        assert p.corrector_kernel == ckernel, (p.corrector_kernel, ckernel)
        response = p.load_kernel != "none"
        assert response == (kernel != "mesh_front")
        if kernel == "fused2d":  # both load routes of the fused plans: substitution in process, the blocked family in the child
            assert p.load_kernel == ("blocked" if group == "blocked_loads" else "fused2d_subst"), p.load_kernel
        for fi, (family, mf) in enumerate(R.DERIVED_FAMILIES):
            coef, M, _ = R.case_inputs(cs, family or R.top_family(cs[1]), mf)
            calls = _load_calls(p, coef, M, inp) if group == "blocked_loads" else _derived_calls(p, coef, M, inp, response)
            for name, v in calls.items():
                out[f"d|{cid}|{fi}|{name}"] = v
        if case in R.DERIVED_SWEEP_CASES and group == "default":
            coef, M, _ = R.case_inputs(cs, "log2", "mild")
            for k, j in R.DERIVED_SWEEP_KJ:
                scaled = dict(inp, loads=inp["loads"] * 2.0**k)
                for name, v in _derived_calls(p, coef * 2.0**k, M * 2.0**j, scaled, response).items():
                    out[f"dsw|{cid}|{k}|{j}|{name}"] = v
            for i in R.DERIVED_SWEEP_DIR:
                s = p.sensitivities(coef, M, directions=inp["directions"] * 2.0**i)
                out[f"ddir|{cid}|{i}|dA"], out[f"ddir|{cid}|{i}|info"] = s.dA, s.info
                if response:
                    s2 = p.second_sensitivities(coef, M, directions=inp["directions"] * 2.0**i, first=True)
                    assert np.array_equal(s2.dA, s.dA)
                    out[f"ddir|{cid}|{i}|d2A"], out[f"ddir|{cid}|{i}|info"] = s2.d2A, np.maximum(s.info, s2.info)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# pivot contract: localized failures
# ------------------------------------------------------------------------------------------------------------------------------

# (group, kernel, kind, dim, n, flags) and the mesh cases
PIVOT_CASES = [("default", "fused2d", "poisson", 2, 5, 0), ("default", "fused2d", "poisson", 2, 17, 0),
               ("default", "small_wave", "elasticity", 2, 10, 0), ("default", "small_wave", "poisson", 3, 6, 0),
               ("default", "small_fused", "poisson", 3, 7, 0), ("default", "multifrontal", "elasticity", 3, 5, 0),
               ("plane", "blocked", "poisson", 3, 6, 0)]
PIVOT_MESH = [R.MESH_CASES[0], R.MESH_CASES[2]]
# doctored copies of good cell 0: (name, factor on the changed element).  -100 x: indefinite; -0.25 x and 0 x: still SPD (classified by the
# test from the eigenvalues of the pinned float64 matrix, both classes must occur)
FACTORS = (("neg100", -100.0), ("negq", -0.25), ("zero", 0.0))


def pivot_elements(cells_p: np.ndarray, n_nodes: int, seed: int) -> list:
    """The six changed elements of a case: the first element, one at the last (gauge) periodic node, one at node 0, three seeded random."""
    at = lambda node: int(np.nonzero((cells_p == node).any(axis=1))[0][-1])  # noqa: E731
    rng = np.random.default_rng(seed)
    return [0, at(n_nodes - 1), at(0)] + [int(e) for e in rng.choice(cells_p.shape[0], 3, replace=False)]


def pivot_batches(kind: str, cells_p: np.ndarray, n_nodes: int, good: np.ndarray, M, n_iso: int = 1) -> dict:
    """Batches of 12 cells: the 6 good cells at even positions, 6 doctored copies of good cell 0 at odd positions.

    name -> (coef[12, ...], M[12, d, d] or None, changed elements).  'neg100' / 'negq' / 'zero': the six elements times a factor;
    'isolated': all elements of one node zero (an exactly zero pivot; never node 0 or the last node, the gauge of the structured routes;
    ``n_iso`` = 2 nodes on mesh plans, whose gauge node is the library's choice: one of the two is not it); 'nan' / 'inf': one element NaN / +Inf;
    'nanM': one NaN entry in the M of the doctored cells."""
    seed = R.case_seed(kind, cells_p.shape, n_nodes)
    els = pivot_elements(cells_p, n_nodes, seed)
    rng = np.random.default_rng(seed + 1)

    def batch():
        c = np.empty((12,) + good.shape[1:])
        c[0::2] = good
        c[1::2] = good[0]
        return c

    MM = None
    if M is not None:
        MM = np.empty((12,) + M.shape[1:])
        MM[0::2] = M
        MM[1::2] = M[0]
    out = {}
    for name, f in FACTORS:
        c = batch()
        for i, e in enumerate(els):
            c[1 + 2 * i, e] *= f
        out[name] = (c, MM, els)
    c = batch()
    nodes = rng.choice(np.arange(1, n_nodes - 1), (6, n_iso), replace=False)
    for i, v in enumerate(nodes):
        c[1 + 2 * i, np.isin(cells_p, v).any(axis=1)] = 0.0
    out["isolated"] = (c, MM, nodes)
    for name, val in (("nan", np.nan), ("inf", np.inf)):
        c = batch()
        for i, e in enumerate(els):
            c[(1 + 2 * i, e) + ((0,) if c.ndim == 3 else ())] = val
        out[name] = (c, MM, els)
    if M is not None:
        Mb = MM.copy()
        for i in range(6):
            Mb[1 + 2 * i].flat[i % Mb[0].size] = np.nan
        out["nanM"] = (batch(), Mb, els)
    return out


def pivot_inputs_structured(kind, dim, n):
    from oracle import hommx_oracle as O

    ne = (2 if dim == 2 else 6) * n**dim
    seed = R.case_seed("pivot", kind, dim, n)
    good = R.coefficients(kind, dim, ne, "log2", 6, seed)
    M = R.stratification(dim, 6, seed)
    cells_p = O.periodic_master_map(dim, n)[O.unit_cell_mesh(dim, n)[1]]
    return good, M, cells_p, n**dim


def pivot_inputs_mesh(kind, builder, args):
    msh = R.mesh_of(builder, args)
    seed = R.case_seed("pivot", kind, builder, args)
    dim = msh.topology.dim
    good = R.coefficients(kind, dim, msh.num_cells, "log2", 6, seed)
    M = R.stratification(dim, 6, seed)
    x, cells, tp = R.mesh_arrays(msh)
    return msh, good, M, tp[cells], int(tp.max()) + 1


def _run_pivot(p, kind, cells_p, n_nodes, good, M, key, out, n_iso=1):
    A0, i0 = p.solve(good, M, return_info=True)
    out[f"goodA|{key}"], out[f"goodinfo|{key}"] = A0, i0
    for name, (c, MM, _) in pivot_batches(kind, cells_p, n_nodes, good, M, n_iso).items():
        A, info = p.solve(c, MM, return_info=True)
        out[f"A|{key}|{name}"], out[f"info|{key}|{name}"] = A, info


def run_pivot_group(group: str) -> dict:
    out = {}
    for g, kernel, kind, dim, n, flags in PIVOT_CASES:
        if g != group:
            continue
        good, M, cells_p, nn = pivot_inputs_structured(kind, dim, n)
        _run_pivot(_plan(kernel, kind, dim, n, flags), kind, cells_p, nn, good, M, skey(kind, dim, n, flags), out)
    if group == "default":
        for kernel, kind, builder, args, route in PIVOT_MESH:
            msh, good, M, cells_p, nn = pivot_inputs_mesh(kind, builder, args)
            _run_pivot(_mesh_plan(kernel, kind, msh, route), kind, cells_p, nn, good, M, mkey(kind, builder, args, route), out, n_iso=2)
    return out


# second derivatives on the doctored batches: one case per load route (substitution on the fused records with the padded NB = 32, the plane
# elimination behind a small-block plan, the tree's back substitution)
PIVOT_SENS2_CASES = [PIVOT_CASES[1], PIVOT_CASES[2], PIVOT_CASES[5]]


def pivot_sens2_batches(dim: int) -> tuple:
    """The doctored batches of a case: both classes occur in ('neg100', 'negq') on all three; the zero element on the 2D cases only (a long-
    double truth of 3D elasticity n = 5 with its float64 yardstick takes a second, and 'negq' asks for six already)."""
    return ("neg100", "negq", "zero") if dim == 2 else ("neg100", "negq")


def pivot_directions(kind, dim, n, good: np.ndarray) -> np.ndarray:
    """Three seeded directions shared by the cells of a pivot case: a random stream, the indicator of every other element, a second random
    stream.  None is a cell's coefficient: no block vanishes, and every block has a scale of its own."""
    rng = np.random.default_rng(R.case_seed("pivot directions", kind, dim, n))
    every_other = np.zeros(good.shape[1:])
    every_other[::2] = 1.0
    return np.stack([rng.standard_normal(good.shape[1:]), every_other, rng.standard_normal(good.shape[1:])])


def run_pivot_sens2_group(group: str = "default") -> dict:
    """second_sensitivities on the all-good batch (keys good<name>|case) and on the doctored batches (keys <name>|case|batch) of the
    PIVOT_SENS2_CASES: d2A, dA, A, info."""
    out = {}
    for g, kernel, kind, dim, n, flags in PIVOT_SENS2_CASES:
        assert g == group
        good, M, cells_p, nn = pivot_inputs_structured(kind, dim, n)
        p = _plan(kernel, kind, dim, n, flags)
        dirs = pivot_directions(kind, dim, n, good)
        key = skey(kind, dim, n, flags)
        r = p.second_sensitivities(good, M, directions=dirs, first=True)
        out[f"goodd2A|{key}"], out[f"gooddA|{key}"], out[f"goodA|{key}"], out[f"goodinfo|{key}"] = r.d2A, r.dA, r.A_eff, r.info
        batches = pivot_batches(kind, cells_p, nn, good, M)
        for name in pivot_sens2_batches(dim):
            c, MM, _ = batches[name]
            r = p.second_sensitivities(c, MM, directions=dirs, first=True)
            out[f"d2A|{key}|{name}"], out[f"dA|{key}|{name}"], out[f"A|{key}|{name}"], out[f"info|{key}|{name}"] = r.d2A, r.dA, r.A_eff, r.info
    return out


def secant_law(law):
    """The ``SecantLaw`` of the texts of a ``nonlinear_truth.Law``, in the shape the kind takes (for the device and the float64 references)."""
    from hommx_amd.expr import SecantLaw

    a, n = law.texts, len(law.texts)
    kw = {} if law.history_texts is None else {"history": list(law.history_texts)}
    if n == 1:
        return SecantLaw(a[0], **kw)
    if n == 2:
        return SecantLaw(lam=a[0], mu=a[1], **kw)
    if n == 3:
        return SecantLaw([[a[0], a[2]], [a[2], a[1]]], **kw)
    if n == 6 and law.kind == "poisson_matrix":
        return SecantLaw([[a[0], a[3], a[4]], [a[3], a[1], a[5]], [a[4], a[5], a[2]]], **kw)
    return SecantLaw(list(a), **kw)


def criterion(crit):
    """The ``Criterion`` of the text of a ``nonlinear_truth.Crit``."""
    from hommx_amd.expr import Criterion

    return Criterion(crit.text, threshold=crit.threshold, **({"history": 1} if crit.with_history else {}))


# the load route of every load shape of nonlinear_truth: one case per route (group 'blocked_loads': the fused plan on the blocked one)
NONLINEAR_LOAD_ROUTES = {"p2": "fused2d_subst", "e3": "blocked", "mesh_ev3": "mesh_front_subst"}


def nonlinear_plan(shape, n=None, load_solve=True):
    """The plan of a shape of tests/nonlinear_truth.py (those of test_gpu_elem_walk_bits.py; ``n``: another size of the structured cell)."""
    import nonlinear_truth as NT
    from hommx_amd import MicroCellPlan

    dim, kind, n0 = NT.SHAPES[shape]
    if n or n0:
        return MicroCellPlan(dim, n or n0, kind)
    return MicroCellPlan.from_mesh(R.mesh_of(*NT.MESHES[dim]), kind, route="front", load_solve=load_solve)


def nonlinear_sibling(shape, p):
    import nonlinear_truth as NT
    from hommx_amd import MicroCellPlan

    dim, _, n = NT.SHAPES[shape]
    return MicroCellPlan(dim, n, p.tangent_kind) if n else MicroCellPlan.from_mesh(R.mesh_of(*NT.MESHES[dim]), p.tangent_kind, route="front")


SECANT_OUTPUTS = {"coef": "coef", "A": "A_eff", "mean_flux": "mean_flux", "strain": "strain", "flux": "flux", "values": "values",
                  "history": "history", "D": "tangent", "tangent_coef": "tangent_coef", "asymmetry": "asymmetry", "status": "status",
                  "info": "info", "tangent_info": "tangent_info", "rounds": "rounds"}


def secant_outputs(r) -> dict:
    """Cell 0 of a SecantResult under the names of nonlinear_truth."""
    return {k: np.asarray(getattr(r, a)[0]) for k, a in SECANT_OUTPUTS.items() if getattr(r, a) is not None}


def run_nonlinear_group(group: str = "default") -> dict:
    """The load cases of nonlinear_truth on the device: a potential law beside a polarisation and an eigenstrain, ``secant_tangent`` with
    max_iter = the round count of the truth and tol = 0, one cell per call (keys nl|shape|cell|E|name).  group 'blocked_loads' (a child
    process with HOMMX_FUSED_LOADS=0): the fused shape alone, its load route asserted."""
    import nonlinear_truth as NT

    out = {}
    for shape in NT.LOAD_SHAPES:
        p = nonlinear_plan(shape)
        if group == "blocked_loads":
            if p.kernel != "fused2d":
                p.close()
                continue
            assert p.load_kernel == "blocked", p.load_kernel
        else:
            assert p.load_kernel == NONLINEAR_LOAD_ROUTES[shape], (shape, p.load_kernel)
        sib = nonlinear_sibling(shape, p)
        law = secant_law(NT.potential_law(p.kind, p.dim))
        coef, M, xi = NT.inputs(shape, 0, NT.tangent_xi(shape))
        load = NT.load_of(shape, 0)
        for c in range(NT.cells_of(shape)):
            for eig in (False, True):
                rounds = NT.load_reference(shape, c, eig)[0]["rounds"]
                r = p.secant_tangent(coef[c:c + 1], xi[c:c + 1], law, sib, None if M is None else M[c:c + 1], max_iter=rounds, tol=0.0,
                                     fields=True, values=True, return_coef=True, return_tangent_coef=True, P=load[c:c + 1], eigenstrain=eig)
                for name, v in secant_outputs(r).items():
                    out[f"nl|{shape}|{c}|{int(eig)}|{name}"] = v
        sib.close()
        p.close()
    return out


RUNNERS = {"nonlinear": run_nonlinear_group, "accuracy": run_accuracy_group, "pivot": run_pivot_group, "derived": run_derived_group, "pivot_sens2": run_pivot_sens2_group}


def run_in_child(what: str, group: str, tmp_path) -> dict:
    """One fresh child process with the group's environment (one child at a time)."""
    f = os.path.join(str(tmp_path), f"{what}_{group}.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, group, f], env=dict(os.environ, **R.CHILD_ENV[group]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(f) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    np.savez(sys.argv[3], **RUNNERS[sys.argv[1]](sys.argv[2]))
    print("ok")
