"""hommx_loads_source[_device] on an MI355X (-m gpu): user-supplied polarisation loads on the smallest shape of every route against the
NumPy / SciPy reference (tests/loads_ref.py) -- the Levin value, the response of the load solve (energy, total flux, fields, correctors),
the canonical loads as user loads, the two device paths to P_eff against each other, a failing cell, invariance (batch position, chunking,
outputs asked for, device against host entry, sampler form against its stream) -- and the solver classes end to end.

Tolerances: 1e-10 for per-cell reductions, 1e-9 for correctors and fields, each relative to the largest magnitude of
the reference array of that cell; coefficients of contrast 1e2 (recon_ref.random_coef)."""

import contextlib
import functools
import os

import numpy as np
import pytest

import loads_ref as L
from hommx_amd import MicroCellPlan, _lib, fem, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream
from hommx_amd.cell_problem import PeriodicLinearProblem

pytestmark = pytest.mark.gpu

FORCE_BLOCKED = 1  # HOMMX_FLAG_FORCE_BLOCKED
# name -> (dim, n or None on the jittered mesh, kind, route of from_mesh, tensor kernel, corrector kernel, environment at plan creation, flags)
CASES = {
    "fused_16": (2, 8, "poisson", None, "fused2d", "fused2d_subst", {}, 0),  # NB = 16; the load solve through the lazy blocked workspace
    "fused_32": (2, 20, "poisson", None, "fused2d", "fused2d_subst", {}, 0),  # NB = 32; 800 elements: more than one per thread
    "small_wave_2d": (2, 6, "elasticity", None, "small_wave", "blocked", {}, 0),
    "small_wave_3d": (3, 4, "poisson", None, "small_wave", "blocked", {}, 0),
    "small_fused": (3, 8, "poisson", None, "small_fused", "blocked", {}, 0),
    "multifrontal": (3, 5, "elasticity", None, "multifrontal", "multifrontal", {}, 0),  # 750 elements: no multiple of the 512 threads
    "multifrontal_staged": (3, 6, "elasticity", None, "multifrontal", "multifrontal", {"HOMMX_MF_STAGE": "64"}, 0),  # stages inside the fronts
    "multifrontal_levels": (2, 24, "poisson", None, "multifrontal", "multifrontal", {"HOMMX_MF_MIN_B": "8", "HOMMX_NO_SMALL_FUSED": "1"},
                            FORCE_BLOCKED),  # a tree of several levels
    "mesh_tree_2d": (2, None, "elasticity", "tree", "mesh_multifrontal", "mesh_multifrontal", {}, 0),
    "mesh_tree_3d": (3, None, "poisson", "tree", "mesh_multifrontal", "mesh_multifrontal", {}, 0),
    "mesh_front": (2, None, "elasticity", None, "mesh_front", "mesh_front", {}, 0),  # P_eff alone: the load solve is refused
}
SOLVED = [c for c in CASES if c != "mesh_front"]
STRAT = [(c, s) for c in CASES for s in ((True, False) if c.startswith("fused") else (True,))]
NC = 5


@contextlib.contextmanager
def _environment(env):
    """The development knobs are read where a piece of a plan is built -- most when the plan is created, those of the corrector plan of
    the tree routes (HOMMX_MF_STAGE among them) and of a fused plan's blocked workspace by the first call that needs the piece: set them
    until that call has been made (``_plan``)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@functools.lru_cache(maxsize=None)
def _mesh(dim):
    return W.jittered_unit_square(10, 8) if dim == 2 else W.jittered_unit_cube(4, 4, 4)


@functools.lru_cache(maxsize=None)
def _plan(name, recon_mb=None):
    dim, n, kind, route, kernel, corr_kernel, env, flags = CASES[name]
    with _environment(dict(env, **({"HOMMX_RECON_MEM_MB": str(recon_mb)} if recon_mb else {}))):
        p = MicroCellPlan(dim, n, kind, flags=flags) if n else MicroCellPlan.from_mesh(_mesh(dim), kind, route=route)
        # one call of everything the tests use, so that the corrector plan and the load pass are built under this environment
        rng = np.random.default_rng(0)
        r = p.loads(L.random_coef(kind, dim, p.n_el, rng)[None], L.random_loads(rng, 1, p.n_el, p.t), response=name != "mesh_front")
        assert not r.info.any()
    assert p.kernel == kernel and p.corrector_kernel == corr_kernel, (p.kernel, p.corrector_kernel)
    return p


def test_staged_case_is_staged():
    """HOMMX_MF_STAGE = 64 is in force on both plans of `multifrontal_staged`: the tensor plan reports it, with a root front that takes
    several stages (more than 64 unknowns), and the corrector plan -- built by the first corrector call, whose stage size nothing
    reports -- eliminates in another order than the default plan of the same shape: tensors of the corrector pass and correctors,
    canonical and of the loads, agree with it to rounding and differ from it in their bits."""
    import re

    dim, n, kind = CASES["multifrontal_staged"][:3]
    staged, default = _plan("multifrontal_staged"), MicroCellPlan(dim, n, kind)
    assert "stages of 64 unknowns" in staged.route_detail and "stages of 192 unknowns" in default.route_detail
    root = int(re.search(r"root s = (\d+)", staged.route_detail).group(1))
    assert root > 64, staged.route_detail  # mf_stages: more than one stage from 65 unknowns (padded to 96) on
    coef, M, shared, _, _ = _case("multifrontal_staged")
    a, b = staged.loads(coef, shared, M, return_correctors=True), default.loads(coef, shared, M, return_correctors=True)
    _, chi_a = staged.solve(coef, M, return_correctors=True)
    _, chi_b = default.solve(coef, M, return_correctors=True)
    for got, want, what in ((chi_a, chi_b, "canonical correctors"), (a.correctors, b.correctors, "load correctors"), (a.A_eff, b.A_eff, "A_eff")):
        _close(got, want, 1e-9, f"staged against default: {what}")
        assert not np.array_equal(got, want), what


@functools.lru_cache(maxsize=None)
def _case(name, strat=True):
    """NC cells with distinct coefficients (and M), t shared and t per-cell loads, and the reference cells; computed once, read only."""
    dim, n, kind = CASES[name][:3]
    p = _plan(name)
    rng = np.random.default_rng(sorted(CASES).index(name) + 100 * strat)
    coef = np.stack([L.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([L.random_M(dim, rng) for _ in range(NC)]) if strat else None
    shared = L.random_loads(rng, p.t, p.n_el, p.t)
    per_cell = np.stack([L.random_loads(rng, p.t, p.n_el, p.t) for _ in range(NC)])
    refs = [L.structured(kind, dim, n, coef[k], None if M is None else M[k]) if n else
            L.on_mesh(_mesh(dim), kind, coef[k], None if M is None else M[k], p.to_periodic) for k in range(NC)]
    for a in (coef, shared, per_cell) + (() if M is None else (M,)):
        a.setflags(write=False)
    return coef, M, shared, per_cell, refs


def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


# -- (a), (c): against the reference; the Levin value against the direct mean flux ---------------------------------------------------------
@pytest.mark.parametrize("name,strat", STRAT)
def test_response_matches_reference(name, strat):
    p = _plan(name)
    coef, M, shared, per_cell, refs = _case(name, strat)
    for nl in (1, p.t):
        for P in (shared[:nl], per_cell[:, :nl]):
            what = f"{name} n_loads {nl} {'per cell' if P.ndim == 4 else 'shared'}"
            if name == "mesh_front":
                r = p.loads(coef, P, M)
                assert r.energy is None and r.correctors is None and not r.info.any()
                for k, ref in enumerate(refs):
                    Pk = P[k] if P.ndim == 4 else P
                    _close(r.P_eff[k], ref.levin(Pk), 1e-10, f"{what} cell {k} P_eff")
                    _close(r.P_eff[k], ref.solve(Pk)["P_eff"], 1e-10, f"{what} cell {k} P_eff against the direct reference")
                    _close(r.A_eff[k], ref.A, 1e-10, f"{what} cell {k} A_eff")
                continue
            r = p.loads(coef, P, M, fields=True, return_correctors=True)
            assert r.P_eff.shape == (NC, nl, p.t) and r.energy.shape == (NC, nl, nl) and r.strain.shape == (NC, nl, p.n_el, p.t)
            assert not r.info.any()
            assert np.array_equal(r.energy, np.swapaxes(r.energy, 1, 2))
            for k, ref in enumerate(refs):
                want = ref.solve(P[k] if P.ndim == 4 else P)
                _close(r.P_eff[k], want["P_eff"], 1e-10, f"{what} cell {k} P_eff (Levin)")
                _close(r.mean_flux[k], want["P_eff"], 1e-10, f"{what} cell {k} mean total flux")
                _close(r.P_eff[k], r.mean_flux[k], 1e-10, f"{what} cell {k} Levin against the device's direct mean flux")
                _close(r.energy[k], want["energy"], 1e-10, f"{what} cell {k} energy")
                _close(r.max_flux[k], want["max_flux"], 1e-10, f"{what} cell {k} max flux")
                for l in range(nl):  # the element the device names reaches the reference's maximum
                    assert want["norm"][l, r.argmax_element[k, l]] >= want["max_flux"][l] * (1 - 1e-9)
                _close(r.A_eff[k], ref.A, 1e-10, f"{what} cell {k} A_eff")
                _close(r.correctors[k], want["chi"], 1e-9, f"{what} cell {k} correctors")
                _close(r.strain[k], want["eps"], 1e-9, f"{what} cell {k} strain")
                _close(r.flux[k], want["q"], 1e-9, f"{what} cell {k} flux")


def test_mesh_front_refuses_the_load_solve():
    p = _plan("mesh_front")
    coef, M, shared, _, _ = _case("mesh_front")
    for kw in ({"response": True}, {"fields": True}, {"return_correctors": True}):
        with pytest.raises(_lib.HommxLibraryError, match="tree route") as e:
            p.loads(coef, shared, M, **kw)
        assert "code -1" in str(e.value) and 'route="tree"' in str(e.value)


# -- (b): the canonical loads as user loads ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_canonical_loads_reproduce_the_canonical_problem(name):
    """P = material(coef) e_m: chi_l = chi^m, P_eff[m] = A_H[:, m], energy = C0 - A_H."""
    dim, n, kind = CASES[name][:3]
    p = _plan(name)
    coef, M, _, _, refs = _case(name)
    P = np.stack([np.transpose(ref.V, (2, 0, 1)) for ref in refs])  # [cell][m][e][:] = V_e e_m
    A, chi = p.solve(coef, M, return_correctors=True)
    if name == "mesh_front":
        r = p.loads(coef, P, M)
    else:
        r = p.loads(coef, P, M, return_correctors=True)
    for k, ref in enumerate(refs):
        _close(r.P_eff[k], A[k].T, 1e-10, f"{name} cell {k} P_eff = A_H")
        if name != "mesh_front":
            _close(r.correctors[k], chi[k], 1e-9, f"{name} cell {k} correctors")
            _close(r.energy[k], ref.C0 - ref.A, 1e-10, f"{name} cell {k} energy = C0 - A_H")
            _close(r.mean_flux[k], A[k].T, 1e-10, f"{name} cell {k} mean flux = A_H")


# -- (d): a failing cell -------------------------------------------------------------------------------------------------------------------
def _fields_of(r):
    return {k: v for k, v in vars(r).items() if v is not None}


def _assert_equal(a, b, cells=slice(None), other=slice(None)):
    fa, fb = _fields_of(a), _fields_of(b)
    assert fa.keys() == fb.keys()
    for key in fa:
        assert np.array_equal(fa[key][cells], fb[key][other], equal_nan=True), key


@pytest.mark.parametrize("name", list(CASES))
def test_bad_cell_is_flagged_and_isolated(name):
    p = _plan(name)
    coef, M, shared, _, _ = _case(name)
    kw = {} if name == "mesh_front" else {"fields": True, "return_correctors": True}
    good = p.loads(coef, shared, M, **kw)
    broken = coef.copy()
    broken[1] = np.nan
    bad = p.loads(broken, shared, M, **kw)
    assert bad.info[1] != 0 and not bad.info[[0, 2, 3, 4]].any() and not good.info.any()
    assert np.isnan(bad.P_eff[1]).all()
    if kw:
        assert np.isnan(bad.energy[1]).all() and np.isnan(bad.mean_flux[1]).all() and np.isnan(bad.flux[1]).all()
    _assert_equal(bad, good, [0, 2, 3, 4], [0, 2, 3, 4])


# -- (e): batch position, what is asked for, chunking ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_outputs_do_not_depend_on_batch_position_or_on_what_is_asked_for(name):
    p = _plan(name)
    coef, M, shared, per_cell, _ = _case(name)
    kw = {} if name == "mesh_front" else {"fields": True, "return_correctors": True}
    full = p.loads(coef, per_cell, M, **kw)
    perm = [3, 0, 4, 1, 2]
    _assert_equal(p.loads(coef[perm], per_cell[perm], M[perm], **kw), full, other=perm)
    _assert_equal(p.loads(coef[2:3], per_cell[2:3], M[2:3], **kw), full, other=slice(2, 3))
    one = p.loads(coef, per_cell[:, 1:2], M, response=bool(kw))  # a load's outputs do not depend on the loads beside it
    assert np.array_equal(one.P_eff, full.P_eff[:, 1:2])
    if not kw:
        return
    assert np.array_equal(one.mean_flux, full.mean_flux[:, 1:2]) and np.array_equal(one.energy[:, 0, 0], full.energy[:, 1, 1])
    plain, resp = p.loads(coef, per_cell, M), p.loads(coef, per_cell, M, response=True)
    assert plain.energy is None and resp.strain is None and resp.correctors is None
    assert np.array_equal(plain.P_eff, full.P_eff) and np.array_equal(plain.A_eff, full.A_eff)
    for key in ("P_eff", "energy", "mean_flux", "max_flux", "argmax_element"):
        assert np.array_equal(getattr(resp, key), getattr(full, key)), key


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_do_not_depend_on_chunking(name):
    """HOMMX_RECON_MEM_MB = 1 on a second plan.  A chunk of the host entry holds, among the rest, what streams per cell -- the fields
    [2][t][n_el][t] of a response, the per-cell P [t][n_el][t] of a P_eff call --, so twice the cells whose share of that fills 1 MB,
    and one more, make three chunks or more; the device-resident route behind the host entry is the same."""
    dim, n, kind = CASES[name][:3]
    p, small = _plan(name), _plan(name, 1)
    solved = name != "mesh_front"
    nc = 2 * max(1, (1 << 20) // (8 * (2 if solved else 1) * p.t * p.n_el * p.t)) + 1
    rng = np.random.default_rng(5)
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([L.random_coef(kind, dim, 2, rng) for _ in range(nc)])
    M = np.stack([L.random_M(dim, rng) for _ in range(nc)])
    shared = L.random_loads(rng, 2, p.n_el, p.t)
    per_cell = rng.standard_normal((nc, p.t, p.n_el, p.t))
    stream, coef = CoefStream.two_phase(mask, values), values[:, mask.astype(int)]
    kw = {"fields": True, "return_correctors": True} if solved else {}
    want = p.loads(stream, per_cell, M, **kw)
    assert not want.info.any() and np.isfinite(want.P_eff).all()
    _assert_equal(small.loads(stream, per_cell, M, **kw), want)
    _assert_equal(small.loads(coef, shared, M, response=solved), p.loads(coef, shared, M, response=solved))


# -- (f): a sampler form against its expanded stream -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_two_phase_stream_equals_its_element_stream_bitwise(name):
    dim, n, kind = CASES[name][:3]
    p = _plan(name)
    _, M, shared, _, _ = _case(name)
    rng = np.random.default_rng(11)
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([L.random_coef(kind, dim, 2, rng) for _ in range(NC)])
    kw = {} if name == "mesh_front" else {"fields": True, "return_correctors": True}
    want = p.loads(values[:, mask.astype(int)], shared, M, **kw)
    assert not want.info.any() and np.isfinite(want.P_eff).all()
    _assert_equal(p.loads(CoefStream.two_phase(mask, values), shared, M, **kw), want)


# -- (g): the device entry against the host entry -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("per_cell", [False, True])
def test_device_entry_equals_host_entry(name, per_cell):
    import torch

    p = _plan(name)
    coef, M, shared, cell_loads, _ = _case(name)
    P = cell_loads if per_cell else shared
    solved = name != "mesh_front"
    want = p.loads(coef, P, M, fields=solved, return_correctors=solved)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))  # a copy: the cached case is read only
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    t, nl = p.t, p.t
    out = {"P_eff": empty(NC, nl, t), "A_eff": empty(NC, t, t), "info": empty(NC, dtype=torch.int32)}
    if solved:
        out.update(energy=empty(NC, nl, nl), stats=empty(NC, nl, t + 2), strain=empty(NC, nl, p.n_el, t), flux=empty(NC, nl, p.n_el, t),
                   correctors=empty(NC, nl, want.correctors.shape[2]))
    ptr = lambda key: out[key].data_ptr() if key in out else None
    p.loads_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nl, upload(P), ptr("P_eff"), per_cell, ptr("A_eff"), ptr("info"),
                   ptr("energy"), ptr("stats"), ptr("strain"), ptr("flux"), ptr("correctors"), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for key in ("P_eff", "A_eff", "info") + (("energy", "strain", "flux", "correctors") if solved else ()):
        assert np.array_equal(got[key], getattr(want, key)), key
    if solved:
        assert np.array_equal(got["stats"][:, :, :t], want.mean_flux) and np.array_equal(got["stats"][:, :, t], want.max_flux)
        assert np.array_equal(got["stats"][:, :, t + 1], want.argmax_element)


# -- end to end ------------------------------------------------------------------------------------------------------------------------------
def _shift_identity(h, P, u0, g, what):
    """P = material(A) E0 with u0 the interpolant of E0 x: solve() with the polarisation and data g = (solve() without it and data g + u0)
    - u0; returns the polarised solution."""
    V = h.function_space
    d = h._tdim
    bnd = fem.locate_dofs_geometrical(V, lambda x: np.any([np.isclose(x[k], 0) | np.isclose(x[k], 1) for k in range(d)], axis=0))

    def solve(data):
        gf = fem.Function(V)
        gf.interpolate(data)
        h.set_boundary_conditions(fem.dirichletbc(gf, bnd, V))
        return h.solve().x.array.copy()

    shifted = solve(lambda X: g(X) + u0(X))
    h.set_polarisation(P)
    with_P = solve(g)
    w = fem.Function(V)
    w.interpolate(u0)
    _close(with_P, shifted - w.x.array, 1e-9, what)
    assert not h.cell_info.any()
    return with_P


def test_poisson_hmm_shift_identity():
    E0 = np.array([0.7, -0.4])
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.02 * (1.0 + 4.0 * x[0]), lambda x: 0.1 + 0.05 * x[1])
    h = hmm.PoissonHMM(Mm.create_unit_square(8, 8), tp, lambda x: 1.0 + x[0], Mm.create_unit_square(8, 8), 0.01)
    _shift_identity(h, lambda x, y: [tp(x, y) * E0[0], tp(x, y) * E0[1]], lambda X: E0 @ X[:2], lambda X: 0.3 * X[0] * X[1], "poisson hmm")
    assert h._plan.kernel == "fused2d"
    _close(h.effective_polarisation, h.effective_tensors @ E0, 1e-10, "P_eff = A_H E0")
    # the response: mean total flux = P_eff; micro flux under the macro solution plus the polarisation, by linearity
    r = h.load_response(cells=[3, 77], fields=True)
    _close(r.mean_flux[:, 0], h.effective_polarisation[[3, 77]], 1e-10, "load_response mean flux")
    total = h.reconstruct(cells=[3, 77], fields=True).flux + r.flux[:, 0]
    assert total.shape == (2, 128, 2) and np.isfinite(total).all()


def test_stratified_elasticity_hmm_shift_identity():
    E = np.array([[0.3, 0.25, -0.1], [0.25, -0.6, 0.2], [-0.1, 0.2, 0.4]])
    lam = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]) + 0.2 * x[1]
    mu = lambda x, y: 0.6 + 0.3 * np.cos(2 * np.pi * y[1]) + 0.1 * x[0]
    tr = np.trace(E)
    P = lambda x, y: [lam(x, y) * tr + 2 * mu(x, y) * E[k, k] for k in range(3)] + [2 * mu(x, y) * E[k, l] for k, l in ((0, 1), (0, 2), (1, 2))]
    h = hmm.LinearElasticityStratifiedHMM(Mm.create_unit_cube(2, 2, 2), lambda x, y: hmm.Lame(lam(x, y), mu(x, y)),
                                          lambda x: np.array([0.0, 0.0, -1.0]), Mm.create_unit_cube(4, 4, 4), 0.01,
                                          lambda x: np.array([[1.0, 0.1, 0.05], [0.2, 0.9, 0.2], [-0.1, 0.15, 1.1]]), quadrature_degree=3)
    _shift_identity(h, P, lambda X: E @ X[:3], lambda X: np.stack([0.1 * X[1] ** 2, 0.2 * X[0] * X[2], 0.05 * X[2]]), "stratified elasticity hmm")
    voigt = np.array([E[0, 0], E[1, 1], E[2, 2], 2 * E[0, 1], 2 * E[0, 2], 2 * E[1, 2]])
    _close(h.effective_polarisation, h.effective_tensors @ voigt, 1e-10, "P_eff = C_H : E0")


@pytest.mark.parametrize("which", ["structured", "jittered"])
def test_periodic_linear_problem_with_loads(which):
    from hommx_amd.cell_problem import create_periodic_boundary_conditions

    msh = Mm.create_unit_square(7, 7) if which == "structured" else W.jittered_unit_square(9, 7)
    kind, t, bs = "elasticity", 3, 2
    rng = np.random.default_rng(2)
    coef, M = L.random_coef(kind, 2, msh.num_cells, rng), L.random_M(2, rng)
    P = L.random_loads(rng, t + 1, msh.num_cells, t)  # more loads than one call takes
    mpc = create_periodic_boundary_conditions(fem.FunctionSpace(msh, bs))
    prob = PeriodicLinearProblem(kind, coef, mpc, M, loads=P)
    canon = prob.solve()
    ref = L.on_mesh(msh, kind, coef, M, mpc.to_periodic)
    want = ref.solve(P)
    at_vertices = lambda chi: chi.reshape(-1, ref.nn, bs)[:, mpc.to_periodic].reshape(len(chi), -1)
    assert len(canon) == t and len(prob.load_correctors) == t + 1 and prob.info == 0
    _close(np.stack([f.x.array for f in canon]), at_vertices(ref.chi_canon), 1e-9, f"{which} canonical functions")
    _close(np.stack([f.x.array for f in prob.load_correctors]), at_vertices(want["chi"]), 1e-9, f"{which} load correctors")
    _close(prob.effective_polarisation, want["P_eff"], 1e-10, f"{which} effective polarisation")
    _close(prob.effective_tensor, ref.A, 1e-10, f"{which} effective tensor")
