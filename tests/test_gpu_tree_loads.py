"""Load solves of the tree routes by substitution on the kept fronts (HOMMX_FLAG_TREE_LOADS / HOMMX_MESH_FLAG_TREE_LOADS; load routes
"multifrontal_subst" / "mesh_multifrontal_subst"; csrc/multifrontal.hip: mf_load_correctors) on an MI355X (-m gpu).

The shapes are the tree cases of tests/test_gpu_loads.py, the smallest at which the forward pass can go wrong, each with a flagged and an
unflagged plan (the parent's route: one more elimination with the load rows overridden):

  multifrontal          3D elasticity 5^3, default stages
  multifrontal_staged   3D elasticity 6^3 with HOMMX_MF_STAGE = 64: several stages inside a front
  multifrontal_levels   2D Poisson 24^2 on the tree (HOMMX_MF_MIN_B = 8, HOMMX_NO_SMALL_FUSED): many levels, bs = 1
  mesh_tree_2d          2D elasticity (bs = 2) on the jittered 9 x 7 square of tests/stream_order_gpu.py
  mesh_tree_3d          3D Poisson on its jittered 3 x 4 x 3 cube; its 36 nodes are ONE front under the default leaf size, so the plan is
                        created with HOMMX_MF_LEAF = 8: five fronts in four groups

``test_shapes_have_fronts_with_children_and_a_parent`` holds every shape to three groups or more before anything leans on it.

a. routes         the flagged names of both families, the unflagged names, no name changes where the route is no tree
b. accuracy       loads() against tests/loads_ref.py and against the unflagged plan, the tolerances of tests/test_gpu_loads.py (1e-10
                  per-cell reductions, 1e-9 correctors and fields, of the cell's largest reference magnitude); the canonical loads as
                  user loads; Levin against the direct mean flux
c. callers        second_sensitivities against tests/sens2_ref.py (1e-9, bitwise symmetric); criterion and four secant rounds with a
                  load against the unflagged plan (1e-9 of the largest entry, test_gpu_secant_load.py case c); A_eff, info and the
                  canonical correctors bitwise those of the unflagged plan
d. invariances    bitwise: batch position, chunking (the derived chunk and the arena cap), HOMMX_MF_STREAMS = 1, the outputs asked
                  for, host against device entry, one load against the same load with others beside it
e. failure        a cell with a negative coefficient keeps its info, no other cell changes a bit
g. end to end     LinearElasticityHMM(tree_loads=True) on 4 x 4 macro cells of n = 5 against the same solver without the keyword
(f, the stream order, is tests/test_gpu_stream_order_tree_loads.py; the accuracy at contrast tests/test_gpu_accuracy_tree_loads.py.)"""

import contextlib
import functools
import os
import re

import numpy as np
import pytest

import loads_ref as L
import sens2_ref as S2
import stream_order_gpu as H
from hommx_amd import MicroCellPlan, hmm, mesh as Mm
from hommx_amd.batch import CoefStream, mesh_analyze_tree

pytestmark = pytest.mark.gpu

FORCE_BLOCKED = 1  # HOMMX_FLAG_FORCE_BLOCKED
# name -> (dim, n or None on the mesh of stream_order_gpu, kind, route of the load solve without the flag, environment at plan creation, flags)
CASES = {
    "multifrontal": (3, 5, "elasticity", "multifrontal", {}, 0),
    "multifrontal_staged": (3, 6, "elasticity", "multifrontal", {"HOMMX_MF_STAGE": "64"}, 0),
    "multifrontal_levels": (2, 24, "poisson", "multifrontal", {"HOMMX_MF_MIN_B": "8", "HOMMX_NO_SMALL_FUSED": "1"}, FORCE_BLOCKED),
    "mesh_tree_2d": (2, None, "elasticity", "mesh_multifrontal", {}, 0),
    "mesh_tree_3d": (3, None, "poisson", "mesh_multifrontal", {"HOMMX_MF_LEAF": "8"}, 0),
}
NC = 5
FULL = {"fields": True, "return_correctors": True}


@contextlib.contextmanager
def environment(env):
    """The development knobs are read where a piece of a plan is built (tests/test_gpu_loads.py, ``_environment``): set until the first
    call of everything the tests use has been made."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def new_plan(name, flagged, **more):
    """A plan of CASES[name] under its environment and ``more``, warmed by one call of every entry the tests use so that the corrector
    plan is built under that environment too."""
    dim, n, kind, route, env, flags = CASES[name]
    with environment(dict(env, **more)):
        p = (MicroCellPlan(dim, n, kind, flags=flags, tree_loads=flagged) if n else
             MicroCellPlan.from_mesh(H.mesh(dim), kind, route="tree", tree_loads=flagged))
        rng = np.random.default_rng(0)
        r = p.loads(L.random_coef(kind, dim, p.n_el, rng)[None], L.random_loads(rng, 1, p.n_el, p.t), response=True)
        assert not r.info.any()
    assert p.kernel == route and p.corrector_kernel == route, (p.kernel, p.corrector_kernel)
    assert p.load_kernel == (route + "_subst" if flagged else route), p.load_kernel
    return p


@functools.lru_cache(maxsize=None)
def plan(name, flagged=True):
    return new_plan(name, flagged)


@functools.lru_cache(maxsize=None)
def case(name, strat=True):
    """NC cells with distinct coefficients (and M), t shared and t per-cell loads, and the reference cells; computed once, read only."""
    dim, n, kind = CASES[name][:3]
    p = plan(name)
    rng = np.random.default_rng(sorted(CASES).index(name) + 100 * strat + 7000)
    coef = np.stack([L.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([L.random_M(dim, rng) for _ in range(NC)]) if strat else None
    shared = L.random_loads(rng, p.t, p.n_el, p.t)
    per_cell = np.stack([L.random_loads(rng, p.t, p.n_el, p.t) for _ in range(NC)])
    refs = [L.structured(kind, dim, n, coef[k], None if M is None else M[k]) if n else
            L.on_mesh(H.mesh(dim), kind, coef[k], None if M is None else M[k], p.to_periodic) for k in range(NC)]
    for a in (coef, shared, per_cell) + (() if M is None else (M,)):
        a.setflags(write=False)
    return coef, M, shared, per_cell, refs


def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


def _fields_of(r):
    return {k: v for k, v in vars(r).items() if isinstance(v, np.ndarray)}


def _assert_equal(a, b, cells=slice(None), other=slice(None)):
    fa, fb = _fields_of(a), _fields_of(b)
    assert fa.keys() == fb.keys()
    for key in fa:
        assert np.array_equal(fa[key][cells], fb[key][other], equal_nan=True), key


# -- the shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_shapes_have_fronts_with_children_and_a_parent(name):
    """Three groups or more: groups are levels of the tree (or shapes at one level), so some front has both children and a parent."""
    dim, n, kind, _, env, _ = CASES[name]
    if n:
        m = re.search(r"(\d+) fronts in (\d+) groups", plan(name).route_detail)
        fronts, groups = int(m.group(1)), int(m.group(2))
    else:
        with environment(env):
            r = mesh_analyze_tree(H.mesh(dim), kind)
        fronts, groups = r["n_fronts"], r["n_groups"]
        parent = np.asarray(r["parent"])
        inner = [f for f in range(fronts) if parent[f] >= 0 and (parent == f).any()]
        assert inner, parent  # a front with a parent and a child
    print(name, fronts, "fronts in", groups, "groups")
    assert groups >= 3 and fronts >= groups, (name, fronts, groups)


def test_staged_case_has_a_front_of_two_stages():
    """HOMMX_MF_STAGE = 64: a front of more than 64 eliminated unknowns (padded to 96 or more) takes two stages or more (mf_stages);
    the root is one, and the plan reports both numbers."""
    detail = plan("multifrontal_staged").route_detail
    assert "stages of 64 unknowns" in detail, detail
    root = int(re.search(r"root s = (\d+)", detail).group(1))
    assert root > 64, detail


# -- a. routes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_route_names(name):
    route = CASES[name][3]
    assert plan(name, True).load_kernel == route + "_subst" and plan(name, False).load_kernel == route
    assert plan(name, True).kernel == plan(name, False).kernel == plan(name, True).corrector_kernel == route


def test_a_flag_changes_no_name_off_the_tree(monkeypatch):
    for args, kw, names in (((2, 6, "elasticity"), {}, ("small_wave", "blocked", "blocked")),
                            ((2, 8, "poisson"), {}, ("fused2d", "fused2d_subst", "fused2d_subst"))):
        for flagged in (False, True):
            p = MicroCellPlan(*args, tree_loads=flagged, **kw)
            assert (p.kernel, p.corrector_kernel, p.load_kernel) == names, (args, flagged)
            p.close()
    for load_solve, load in ((False, "none"), (True, "mesh_front_subst")):
        for flagged in (False, True):
            p = MicroCellPlan.from_mesh(H.mesh(2), "elasticity", load_solve=load_solve, tree_loads=flagged)
            assert (p.kernel, p.corrector_kernel, p.load_kernel) == ("mesh_front", "mesh_front", load), (load_solve, flagged)
            p.close()
    monkeypatch.setenv("HOMMX_MF_CORR", "0")  # the correctors leave the tree: there are no kept fronts to substitute on
    p = MicroCellPlan(3, 5, "elasticity", tree_loads=True)
    assert (p.kernel, p.corrector_kernel, p.load_kernel) == ("multifrontal", "blocked", "blocked")
    p.close()


# -- b. accuracy -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [True, False], ids=["M", "no_M"])
@pytest.mark.parametrize("name", list(CASES))
def test_b_response_matches_reference_and_the_unflagged_plan(name, strat):
    p, q = plan(name, True), plan(name, False)
    coef, M, shared, per_cell, refs = case(name, strat)
    _, chi = q.solve(coef, M, return_correctors=True)
    assert np.array_equal(p.solve(coef, M, return_correctors=True)[1], chi)  # the canonical correctors: the same pass
    for nl in (1, p.t):
        for P in (shared[:nl], per_cell[:, :nl]):
            what = f"{name} n_loads {nl} {'per cell' if P.ndim == 4 else 'shared'}"
            r, u = p.loads(coef, P, M, **FULL), q.loads(coef, P, M, **FULL)
            assert r.P_eff.shape == (NC, nl, p.t) and r.energy.shape == (NC, nl, nl) and r.strain.shape == (NC, nl, p.n_el, p.t)
            assert not r.info.any() and np.array_equal(r.info, u.info)
            assert np.array_equal(r.A_eff, u.A_eff) and np.array_equal(r.P_eff, u.P_eff)  # the canonical pass, and Levin's value on it
            for k, ref in enumerate(refs):
                want = ref.solve(P[k] if P.ndim == 4 else P)
                _close(r.P_eff[k], want["P_eff"], 1e-10, f"{what} cell {k} P_eff (Levin)")
                _close(r.mean_flux[k], want["P_eff"], 1e-10, f"{what} cell {k} mean total flux")
                _close(r.P_eff[k], r.mean_flux[k], 1e-10, f"{what} cell {k} Levin against the device's direct mean flux")
                _close(r.energy[k], want["energy"], 1e-10, f"{what} cell {k} energy")
                _close(r.max_flux[k], want["max_flux"], 1e-10, f"{what} cell {k} max flux")
                for l in range(nl):
                    assert want["norm"][l, r.argmax_element[k, l]] >= want["max_flux"][l] * (1 - 1e-9)
                _close(r.A_eff[k], ref.A, 1e-10, f"{what} cell {k} A_eff")
                _close(r.correctors[k], want["chi"], 1e-9, f"{what} cell {k} correctors")
                _close(r.strain[k], want["eps"], 1e-9, f"{what} cell {k} strain")
                _close(r.flux[k], want["q"], 1e-9, f"{what} cell {k} flux")
                _close(r.energy[k], u.energy[k], 1e-10, f"{what} cell {k} energy against the unflagged plan")
                _close(r.mean_flux[k], u.mean_flux[k], 1e-10, f"{what} cell {k} mean flux against the unflagged plan")
                _close(r.correctors[k], u.correctors[k], 1e-9, f"{what} cell {k} correctors against the unflagged plan")
                _close(r.strain[k], u.strain[k], 1e-9, f"{what} cell {k} strain against the unflagged plan")
                _close(r.flux[k], u.flux[k], 1e-9, f"{what} cell {k} flux against the unflagged plan")


@pytest.mark.parametrize("name", list(CASES))
def test_b_canonical_loads_reproduce_the_canonical_problem(name):
    """P = material(coef) e_m: chi_l = chi^m -- the border rows of the elimination carry exactly this forward pass."""
    p = plan(name)
    coef, M, _, _, refs = case(name)
    P = np.stack([np.transpose(ref.V, (2, 0, 1)) for ref in refs])  # [cell][m][e][:] = V_e e_m
    A, chi = p.solve(coef, M, return_correctors=True)
    r = p.loads(coef, P, M, return_correctors=True)
    for k, ref in enumerate(refs):
        _close(r.correctors[k], chi[k], 1e-9, f"{name} cell {k} correctors")
        _close(r.P_eff[k], A[k].T, 1e-10, f"{name} cell {k} P_eff = A_H")
        _close(r.energy[k], ref.C0 - ref.A, 1e-10, f"{name} cell {k} energy = C0 - A_H")
        _close(r.mean_flux[k], A[k].T, 1e-10, f"{name} cell {k} mean flux = A_H")


# -- c. the callers --------------------------------------------------------------------------------------------------------------------------
def _directions(name):
    coef = case(name)[0]
    rng = np.random.default_rng(31 + sorted(CASES).index(name))
    half = np.zeros(coef.shape[1:])
    half[::2] = 1.0
    return np.stack([coef[0], rng.standard_normal(coef.shape[1:]), half, rng.standard_normal(coef.shape[1:])])  # four shared directions


@pytest.mark.parametrize("name", list(CASES))
def test_c_second_sensitivities(name):
    dim, n, kind = CASES[name][:3]
    p, q = plan(name, True), plan(name, False)
    coef, M, _, _, _ = case(name)
    dirs = _directions(name)
    r, u = p.second_sensitivities(coef, M, directions=dirs, first=True), q.second_sensitivities(coef, M, directions=dirs, first=True)
    assert not r.info.any() and np.array_equal(r.info, u.info) and np.array_equal(r.A_eff, u.A_eff) and np.array_equal(r.dA, u.dA)
    assert np.array_equal(r.d2A, np.swapaxes(r.d2A, 3, 4)) and np.array_equal(r.d2A, np.swapaxes(r.d2A, 1, 2))  # bitwise symmetric
    for k in range(NC):
        cell = S2.structured(kind, dim, n, coef[k], M[k]) if n else S2.on_mesh(H.mesh(dim), kind, coef[k], M[k])
        want = S2.second_derivatives(cell, dirs)
        _close(r.d2A[k], want, 1e-9, f"{name} cell {k} d2A")
        _close(r.d2A[k], u.d2A[k], 1e-9, f"{name} cell {k} d2A against the unflagged plan")


@functools.lru_cache(maxsize=None)
def _state(name):
    """What a law and a criterion read beside the cells: macro strains, rows (midpoint), points, one load per cell of order 0.3."""
    p = plan(name)
    rng = np.random.default_rng(9100 + sorted(CASES).index(name))
    d = {"xi": rng.standard_normal((NC, p.t)), "rows": rng.integers(-8, 9, (NC, 3)) / 8.0, "points": rng.integers(0, 17, (p.n_el, p.dim)) / 16.0,
         "load": 0.3 * rng.standard_normal((NC, p.n_el, p.t)) + 0.2 * rng.standard_normal((NC, 1, p.t))}
    for a in d.values():
        a.setflags(write=False)
    return d


@pytest.mark.parametrize("eigenstrain", [False, True], ids=["P", "E"])
@pytest.mark.parametrize("name", list(CASES))
def test_c_criterion_and_four_secant_rounds(name, eigenstrain):
    from hommx_amd.expr import Criterion
    from test_gpu_secant import soft_law

    p, q = plan(name, True), plan(name, False)
    coef, M, _, _, _ = case(name)
    d = _state(name)
    kw = dict(rows=d["rows"], points=d["points"], P=d["load"], eigenstrain=eigenstrain)
    r, u = (x.criterion(coef, d["xi"], Criterion("e[0]"), M, fields=True, values=True, **kw) for x in (p, q))
    assert np.array_equal(r.A_eff, u.A_eff) and np.array_equal(r.info, u.info) and not r.info.any()
    for key in ("strain", "flux", "values"):
        _close(getattr(r, key), getattr(u, key), 1e-9, f"{name} criterion {key}")
    law = soft_law(p.kind, p.dim)
    first = [x.secant(coef, d["xi"], law, M, max_iter=1, **kw) for x in (p, q)]
    assert np.array_equal(first[0].A_eff, first[1].A_eff) and np.array_equal(first[0].info, first[1].info)  # round one: the same canonical pass
    r, u = (x.secant(coef, d["xi"], law, M, max_iter=4, tol=0.0, return_coef=True, **kw) for x in (p, q))
    assert np.array_equal(r.rounds, np.full(NC, 4)) and np.array_equal(r.status, u.status) and not r.info.any()
    for c in range(NC):
        dc = np.abs(r.coef[c] - u.coef[c]).max() / np.abs(u.coef[c]).max()
        dA = np.abs(r.A_eff[c] - u.A_eff[c]).max() / np.abs(u.A_eff[c]).max()
        df = np.abs(r.mean_flux[c] - u.mean_flux[c]).max() / np.abs(u.mean_flux[c]).max()
        print(f"{name} cell {c}: fourth iterate against the unflagged plan, coef {dc:.3e}, A_eff {dA:.3e}, mean_flux {df:.3e}")
        assert dc <= 1e-9 and dA <= 1e-9 and df <= 1e-9


# -- d. invariances, bitwise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_d_batch_position_outputs_asked_for_and_loads_beside(name):
    p = plan(name)
    coef, M, _, per_cell, _ = case(name)
    full = p.loads(coef, per_cell, M, **FULL)
    perm = [3, 0, 4, 1, 2]
    _assert_equal(p.loads(coef[perm], per_cell[perm], M[perm], **FULL), full, other=perm)
    _assert_equal(p.loads(coef[2:3], per_cell[2:3], M[2:3], **FULL), full, other=slice(2, 3))
    one = p.loads(coef, per_cell[:, 1:2], M, **FULL)  # a load's outputs do not depend on the loads beside it
    assert np.array_equal(one.P_eff, full.P_eff[:, 1:2]) and np.array_equal(one.mean_flux, full.mean_flux[:, 1:2])
    assert np.array_equal(one.energy[:, 0, 0], full.energy[:, 1, 1]) and np.array_equal(one.correctors, full.correctors[:, 1:2])
    assert np.array_equal(one.strain, full.strain[:, 1:2]) and np.array_equal(one.flux, full.flux[:, 1:2])
    plain, resp = p.loads(coef, per_cell, M), p.loads(coef, per_cell, M, response=True)
    assert plain.energy is None and resp.strain is None and resp.correctors is None
    assert np.array_equal(plain.P_eff, full.P_eff) and np.array_equal(plain.A_eff, full.A_eff)
    for key in ("P_eff", "energy", "mean_flux", "max_flux", "argmax_element", "A_eff", "info"):
        assert np.array_equal(getattr(resp, key), getattr(full, key)), key


@pytest.mark.parametrize("name", list(CASES))
def test_d_chunking_streams(name):
    """Three more flagged plans.  HOMMX_RECON_MEM_MB = 1: the chunk rule of the reconstruction binds (three chunks or more, as in
    tests/test_gpu_loads.py).  HOMMX_BLOCKED_MEM_GB = 1e-6: an arena of ONE cell, so the arena cap binds -- every chunk is one cell,
    and a chunk of more would be refused by the guard of the load solve, since mf_solve would run it in pieces of one.
    HOMMX_MF_STREAMS = 1 against the default: at 21 cells or more the default plan runs a chunk as two pieces, one on a side stream."""
    dim, n, kind = CASES[name][:3]
    p = plan(name)
    nc = max(21, 2 * max(1, (1 << 20) // (8 * 2 * p.t * p.n_el * p.t)) + 1)
    rng = np.random.default_rng(5)
    coef = np.stack([L.random_coef(kind, dim, p.n_el, rng) for _ in range(nc)])
    M = np.stack([L.random_M(dim, rng) for _ in range(nc)])
    per_cell = rng.standard_normal((nc, p.t, p.n_el, p.t))
    dirs = _directions(name)[1:3]
    want, want2 = p.loads(coef, per_cell, M, **FULL), p.second_sensitivities(coef, M, directions=dirs)
    assert not want.info.any() and np.isfinite(want.correctors).all()
    for env in ({"HOMMX_RECON_MEM_MB": "1"}, {"HOMMX_BLOCKED_MEM_GB": "1e-6"}, {"HOMMX_RECON_MEM_MB": "1", "HOMMX_BLOCKED_MEM_GB": "1e-6"},
                {"HOMMX_MF_STREAMS": "1"}):
        other = new_plan(name, True, **env)
        _assert_equal(other.loads(coef, per_cell, M, **FULL), want)
        _assert_equal(other.second_sensitivities(coef, M, directions=dirs), want2)
        other.close()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("per_cell", [False, True])
def test_d_device_entry_equals_host_entry(name, per_cell):
    import torch

    p = plan(name)
    coef, M, shared, cell_loads, _ = case(name)
    P = cell_loads if per_cell else shared
    want = p.loads(coef, P, M, **FULL)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    t, nl = p.t, p.t
    out = {"P_eff": empty(NC, nl, t), "A_eff": empty(NC, t, t), "info": empty(NC, dtype=torch.int32), "energy": empty(NC, nl, nl),
           "stats": empty(NC, nl, t + 2), "strain": empty(NC, nl, p.n_el, t), "flux": empty(NC, nl, p.n_el, t),
           "correctors": empty(NC, nl, want.correctors.shape[2])}
    ptr = lambda key: out[key].data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    p.loads_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nl, upload(P), ptr("P_eff"), per_cell, ptr("A_eff"), ptr("info"),
                   ptr("energy"), ptr("stats"), ptr("strain"), ptr("flux"), ptr("correctors"), stream=st)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for key in ("P_eff", "A_eff", "info", "energy", "strain", "flux", "correctors"):
        assert np.array_equal(got[key], getattr(want, key)), key
    assert np.array_equal(got["stats"][:, :, :t], want.mean_flux) and np.array_equal(got["stats"][:, :, t], want.max_flux)
    dirs = _directions(name)[1:3]
    want2 = p.second_sensitivities(coef, M, directions=dirs, first=True)
    d2A, dA, A, info = empty(NC, 2, 2, t, t), empty(NC, 2, t, t), empty(NC, t, t), empty(NC, dtype=torch.int32)
    p.second_sensitivities_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), 2, upload(dirs), d2A.data_ptr(), False,
                                  dA.data_ptr(), A.data_ptr(), info.data_ptr(), stream=st)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d2A.cpu().numpy(), want2.d2A) and np.array_equal(dA.cpu().numpy(), want2.dA)
    assert np.array_equal(A.cpu().numpy(), want2.A_eff) and np.array_equal(info.cpu().numpy(), want2.info)


# -- e. failure ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_e_bad_cell_is_flagged_and_isolated(name):
    p, q = plan(name, True), plan(name, False)
    coef, M, shared, _, _ = case(name)
    good = p.loads(coef, shared, M, **FULL)
    broken = coef.copy()
    broken[1] = -broken[1]  # a negative coefficient: the first pivot is not positive
    bad = p.loads(broken, shared, M, **FULL)
    assert bad.info[1] != 0 and not bad.info[[0, 2, 3, 4]].any() and not good.info.any()
    assert np.array_equal(bad.info, q.loads(broken, shared, M, response=True).info)  # the info of the canonical pass, kept
    _assert_equal(bad, good, [0, 2, 3, 4], [0, 2, 3, 4])
    dirs = _directions(name)[1:3]
    good2, bad2 = p.second_sensitivities(coef, M, directions=dirs), p.second_sensitivities(broken, M, directions=dirs)
    assert bad2.info[1] == bad.info[1] and not bad2.info[[0, 2, 3, 4]].any()
    for k in (0, 2, 3, 4):
        assert np.array_equal(bad2.d2A[k], good2.d2A[k]) and np.array_equal(bad2.A_eff[k], good2.A_eff[k])


# -- g. end to end ---------------------------------------------------------------------------------------------------------------------------
def _solver(**kw):
    from hommx_amd import fem

    A = hmm.TwoPhase(lambda y: y[0] < 0.5, lambda x: hmm.Lame(20.0 + 0.0 * x[0], 10.0 + 0.0 * x[0]),
                     lambda x: hmm.Lame(2.0 + 0.0 * x[0], 1.0 + 0.0 * x[0]))
    h = hmm.LinearElasticityHMM(Mm.create_unit_square(4, 4), A, lambda x: np.array([0.0, -8.0]), Mm.create_unit_square(5, 5), 0.05, **kw)
    V = h.function_space
    clamp = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1) | np.isclose(x[1], 0) | np.isclose(x[1], 1))
    h.set_boundary_conditions(fem.dirichletbc(fem.Function(V), clamp, V))
    h.set_eigenstrain(lambda x, y: [0.01 + 0.02 * x[0] + 0.01 * np.sin(2 * np.pi * y[1]), 0.02 + 0.0 * x[0] * y[0], 0.0 * x[0] * y[0]])
    return h


# 2D elasticity of n = 5 has a plane block of 10 unknowns, the one-wave route by default: these knobs put it on the tree, with leaves of
# four nodes so that the 25 nodes make a tree of several levels
E2E_ENV = {"HOMMX_MF_MIN_B": "8", "HOMMX_NO_SMALL_FUSED": "1", "HOMMX_MF_LEAF": "4"}


def test_g_solver_class_end_to_end():
    """solve(), load_response() and solve_nonlinear(load=True) of LinearElasticityHMM(tree_loads=True) against the same solver without
    the keyword, both on the tree route: solve() forms P_eff by Levin's formula on the canonical pass (1e-12 of max |u|, the bound of the
    identity law in case i of test_gpu_secant_load.py); the response to the bounds of tests/test_gpu_loads.py; the nonlinear solution
    within 10 tol, the bound of that file's elasticity case."""
    tol = 1e-8
    law = hmm.SecantLaw(lam="c[0]", mu="c[1]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))")
    got = {}
    with environment(E2E_ENV):
        for flagged in (True, False):
            h = _solver(**({"tree_loads": True} if flagged else {}))
            u = h.solve().x.array.copy()
            r = h.load_response(fields=True)
            v = h.solve_nonlinear(law, max_iter=60, tol=tol, load=True).x.array.copy()
            assert h._plan.kernel == "multifrontal" and h._plan.load_kernel == ("multifrontal_subst" if flagged else "multifrontal")
            m = re.search(r"(\d+) fronts in (\d+) groups", h._plan.route_detail)
            assert int(m.group(2)) >= 3, h._plan.route_detail
            assert h.nonlinear_history[-1] <= tol and len(h.nonlinear_history) > 2 and not h.secant.status.any() and not h.cell_info.any()
            got[flagged] = (u, r, v, h.effective_polarisation.copy())
    (u1, r1, v1, P1), (u0, r0, v0, P0) = got[True], got[False]
    du = np.abs(u1 - u0).max() / np.abs(u0).max()
    dv = np.abs(v1 - v0).max() / np.abs(v0).max()
    print(f"tree_loads end to end: solve {du:.3e}, solve_nonlinear {dv:.3e} of max |u|")
    assert du <= 1e-12 and np.abs(u0).max() > 0
    _close(r1.mean_flux, r0.mean_flux, 1e-10, "load_response mean flux")
    _close(r1.energy, r0.energy, 1e-10, "load_response energy")
    _close(r1.flux, r0.flux, 1e-9, "load_response flux")
    assert dv <= 10 * tol
    assert np.abs(P1 - P0).max() <= 10 * tol * np.abs(P0).max()
    assert np.abs(v0 - u0).max() > 1e-6 * np.abs(u0).max()  # the law matters
