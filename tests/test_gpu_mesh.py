"""The mesh route (hommx_plan_create_mesh, csrc/mesh_front.hip) on an MI355X (-m gpu): structured equivalence with the existing
routes, unstructured accuracy against the test-side reference tests/periodic_fem.py, closed forms, invariance, failure isolation,
device samplers, the solver classes end to end."""

import ctypes as C

import numpy as np
import pytest

import periodic_fem as PF
from hommx_amd import MicroCellPlan, _lib, fem, hmm, mesh as Mm, workloads as W

pytestmark = pytest.mark.gpu

KINDS = ["poisson", "poisson_matrix", "elasticity", "elasticity_voigt"]


def _coef(kind, dim, ne, rng, nc=None):
    shp = () if nc is None else (nc,)
    t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
    if kind == "poisson":
        return rng.uniform(0.5, 2.0, shp + (ne,))
    if kind == "poisson_matrix":
        L = rng.normal(size=shp + (ne, dim, dim)) * 0.3 + np.eye(dim)
        A = L @ np.swapaxes(L, -1, -2)
        return np.stack([A[..., k, l] for k, l in PF.PAIRS[dim]], -1)
    if kind == "elasticity":
        return np.stack([rng.uniform(0.5, 2.0, shp + (ne,)), rng.uniform(0.5, 2.0, shp + (ne,))], -1)
    L = rng.normal(size=shp + (ne, t, t)) * 0.3 + 2 * np.eye(t)
    V = L @ np.swapaxes(L, -1, -2)
    iu = np.triu_indices(t)
    return V[..., iu[0], iu[1]]


def _M(dim, nc, rng):
    return np.eye(dim) + 0.2 * rng.normal(size=(nc, dim, dim))


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_structured_equivalence(kind, dim, rng):
    if dim == 2:
        msh, n = Mm.create_unit_square(16, 16), 16
    else:
        n = 4 if kind.startswith("poisson") else 3
        msh = Mm.create_unit_cube(n, n, n)
    p = MicroCellPlan.from_mesh(msh, kind)
    assert p.kernel == "mesh_front" and p.n_micro is None and 0 < p.front_width <= _lib.MESH_MAX_FRONT
    q = MicroCellPlan(dim, n, kind)
    coef = _coef(kind, dim, msh.num_cells, rng, nc=6)
    for M in (None, _M(dim, 6, rng)):
        A, info = p.solve(coef, M, return_info=True)
        assert np.all(info == 0)
        assert _rel(A, q.solve(coef, M)) < 1e-11


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_unstructured_matches_reference(kind, dim, rng):
    msh = W.jittered_unit_square(12, 9, seed=5) if dim == 2 else W.jittered_unit_cube(3, 4, 3, seed=6)
    p = MicroCellPlan.from_mesh(msh, kind)
    nc = 3
    coef = _coef(kind, dim, msh.num_cells, rng, nc=nc)
    M = _M(dim, nc, rng)
    A, chi, info = p.solve(coef, M, return_info=True, return_correctors=True)
    assert np.all(info == 0)
    bs = 1 if kind.startswith("poisson") else dim
    for c in range(nc):
        ref, chi_r, node = PF.solve_cell(msh, kind, coef[c], M[c])
        assert _rel(A[c], ref) < 1e-10
        mine = chi[c].reshape(p.t, -1, bs)[:, p.to_periodic]
        theirs = chi_r.reshape(p.t, -1, bs)[:, node]
        assert np.allclose(chi[c].reshape(p.t, -1, bs).mean(axis=1), 0.0, atol=1e-13)
        d = mine - theirs
        d -= d.mean(axis=1, keepdims=True)
        assert np.abs(d).max() < 1e-9 * max(1.0, np.abs(theirs).max())


def test_laminate_closed_form():
    layers = [0.3, 0.71]
    msh = W.layered_unit_square(layers, 14, 10, seed=3)
    y = msh.cell_midpoints()[:, 1]
    a = np.where((y > 0.3) & (y < 0.71), 7.5, 0.4)
    vol = msh.cell_volumes()
    p = MicroCellPlan.from_mesh(msh, "poisson")
    A = p.solve(a[None])[0]
    arith = (vol * a).sum()
    harm = 1.0 / (vol / a).sum()
    assert abs(A[0, 0] - arith) < 1e-12 * arith and abs(A[1, 1] - harm) < 1e-12 * arith
    assert abs(A[0, 1]) < 1e-12 * arith and abs(A[1, 0]) < 1e-12 * arith
    # constant coefficient: A_H = A, C_H = C
    assert np.abs(p.solve(np.full((1, msh.num_cells), 2.5))[0] - 2.5 * np.eye(2)).max() < 1e-12
    pe = MicroCellPlan.from_mesh(msh, "elasticity")
    C = pe.solve(np.tile([1.25, 5.0], (1, msh.num_cells, 1)))[0]
    Cv = np.array([[1.25 + 10.0, 1.25, 0.0], [1.25, 11.25, 0.0], [0.0, 0.0, 5.0]])
    assert np.abs(C - Cv).max() < 1e-12 * 11.25


def test_renumbering_and_batch_invariance(rng):
    msh = W.jittered_unit_square(11, 13, seed=8)
    kind = "elasticity"
    coef = _coef(kind, 2, msh.num_cells, rng, nc=5)
    M = _M(2, 5, rng)
    p = MicroCellPlan.from_mesh(msh, kind)
    A = p.solve(coef, M)
    pv = rng.permutation(msh.num_vertices)
    pe = rng.permutation(msh.num_cells)
    inv = np.argsort(pv)
    msh2 = Mm.create_mesh(inv[msh.cells[pe]], msh.geometry.x[pv][:, :2])
    A2 = MicroCellPlan.from_mesh(msh2, kind).solve(coef[:, pe], M)
    assert _rel(A2, A) < 1e-12
    for c in range(5):  # a cell does not depend on the batch it travels in
        assert np.array_equal(p.solve(coef[c : c + 1], M[c : c + 1])[0], A[c])


def test_bad_cells_flagged_neighbours_unaffected(rng):
    msh = W.jittered_unit_square(10, 10, seed=9)
    p = MicroCellPlan.from_mesh(msh, "poisson")
    coef = _coef("poisson", 2, msh.num_cells, rng, nc=6)
    good, ginfo = p.solve(coef, return_info=True)
    bad = coef.copy()
    bad[2] = -1.0
    bad[4, 7] = np.nan
    A, info = p.solve(bad, return_info=True)
    assert info[2] != 0 and info[4] != 0
    for c in (0, 1, 3, 5):
        assert info[c] == 0 and np.array_equal(A[c], good[c])
    assert np.all(ginfo == 0)


def test_samplers_match_host_stream(rng):
    msh = W.jittered_unit_square(12, 10, seed=4)
    p = MicroCellPlan.from_mesh(msh, "poisson")
    yb = msh.cell_midpoints()[:, :2]
    mask = W.wrapped_disc(yb[:, 0], yb[:, 1])
    values = rng.uniform(0.1, 3.0, (7, 2))
    A = p.solve_two_phase(mask, values)
    stream = np.where(mask[None], values[:, 1:2], values[:, 0:1])
    assert np.abs(A - p.solve(stream)).max() < 1e-13 * np.abs(A).max()
    table = np.sin(2 * np.pi * yb[:, 0])
    params = np.stack([rng.uniform(1.5, 2.0, 7), rng.uniform(0.1, 0.5, 7)], 1)
    A = p.solve_separable("affine", table, None, params)
    stream = params[:, :1] + params[:, 1:] * table[None]
    assert np.abs(A - p.solve(stream)).max() < 1e-13 * np.abs(A).max()
    pe = MicroCellPlan.from_mesh(msh, "elasticity")
    lame = rng.uniform(0.5, 2.0, (4, 2, 2))
    A = pe.solve_two_phase(mask, lame)
    stream = np.where(mask[None, :, None], lame[:, 1:2], lame[:, 0:1])
    assert np.abs(A - pe.solve(stream)).max() < 1e-13 * np.abs(A).max()


def _twin_with_reference(h):
    """Same solver, effective tensors from the test-side reference instead of the GPU."""

    def eff(cells):
        coef, kind = h._element_means(cells)
        M = h._stratification(cells)
        out = np.stack([PF.solve_cell(h._cell_mesh, kind, coef[i], None if M is None else M[i])[0] for i in range(len(cells))])
        return out, np.zeros(len(cells), np.int32)

    h._effective_tensors = eff
    return h


def test_poisson_hmm_unstructured_micro():
    def mk():
        msh = Mm.create_unit_square(4, 4)
        h = hmm.PoissonHMM(msh, lambda x, y: 1.1 + x[0] + np.sin(2 * np.pi * y[0]) * 0.5, lambda x: np.ones(x.shape[1]),
                           W.jittered_unit_square(10, 8, seed=1), 2.0**-4, quadrature_degree=0)
        V = h.function_space
        dofs = fem.locate_dofs_topological(V, 1, fem.locate_entities_boundary(msh, 1, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1)))
        h.set_boundary_conditions(fem.dirichletbc(0.0, dofs, V))
        return h

    h = mk()
    assert h.prepare()._plan.kernel == "mesh_front"
    u = h.solve()
    assert np.all(h.cell_info == 0)
    ur = _twin_with_reference(mk()).solve()
    assert np.abs(u.x.array - ur.x.array).max() < 1e-10 * np.abs(ur.x.array).max()
    chi = h.correctors_for_cell(3)
    assert len(chi) == 3 and chi[0].x.array.shape == (h._cell_mesh.num_vertices,)


def test_elasticity_stratified_hmm_unstructured_micro():
    def A(x, y):
        return hmm.Lame(1.0 + 0.0 * y[0], np.where(np.cos(2 * np.pi * y[1]) > 0, 8.0, 0.5))

    def Dt(x):
        return np.array([[1.0, 0.0], [0.3 * np.cos(x[0]), 1.0]])

    def mk():
        msh = Mm.create_rectangle([(0, 0), (1.0, 0.5)], (4, 2))
        h = hmm.LinearElasticityStratifiedHMM(msh, A, lambda x: np.array([0.0, -0.01]), W.layered_unit_square([0.25, 0.75], 8, 8, seed=2),
                                              2.0**-4, Dt)
        V = h.function_space
        clamp = fem.locate_dofs_topological(V, 1, fem.locate_entities_boundary(msh, 1, lambda x: np.isclose(x[0], 0)))
        h.set_boundary_conditions(fem.dirichletbc(np.zeros(2), clamp, V))
        return h

    h = mk()
    u = h.solve()
    assert np.all(h.cell_info == 0)
    ur = _twin_with_reference(mk()).solve()
    assert np.abs(u.x.array - ur.x.array).max() < 1e-10 * np.abs(ur.x.array).max()


def test_poisson_periodic_hmm_unstructured_micro():
    micro = W.jittered_unit_square(9, 11, seed=7)
    A = lambda y: 1.0 / (2.0 + np.cos(2 * np.pi * y[0]))
    h = hmm.PoissonPeriodicHMM(Mm.create_unit_square(4, 4), A, lambda x: np.ones(x.shape[1]), micro, 2.0**-4, quadrature_degree=0)
    AH = h.compute_effective_tensor()
    coef, kind = h._inner._element_means(np.array([0]))
    ref, chi_r, node = PF.solve_cell(micro, kind, coef[0])
    assert _rel(AH, ref) < 1e-10
    for q, f in enumerate(h.correctors):
        d = f.x.array - chi_r[q][node]
        assert np.abs(d - d.mean()).max() < 1e-9 * max(1.0, np.abs(chi_r[q]).max())


def test_multi_refuses_mesh_plans():
    lib = _lib.load()
    comm = C.c_void_p()
    _lib.check(lib.hommx_comm_init_all(C.byref(comm), 1, None), "hommx_comm_init_all")
    try:
        p = MicroCellPlan.from_mesh(W.jittered_unit_square(6, 6), "poisson")
        plans = (C.c_void_p * 1)(p._h.value)
        coef = np.ones((2, p.n_el))
        out = np.zeros((2, 2, 2))
        info = np.zeros(2, np.int32)
        rc = lib.hommx_solve_batch_multi(comm, plans, 2, coef.ctypes.data, None, out.ctypes.data, info.ctypes.data)
        assert rc == -1 and "mesh plan" in _lib.last_error()
    finally:
        lib.hommx_comm_destroy(comm)


def test_periodic_linear_problem_on_mesh(rng):
    from hommx_amd.cell_problem import PeriodicLinearProblem, create_periodic_boundary_conditions

    msh = W.jittered_unit_cube(3, 3, 4, seed=2)
    V = fem.FunctionSpace(msh, 3)
    mpc = create_periodic_boundary_conditions(V)
    coef = _coef("elasticity", 3, msh.num_cells, rng)
    lp = PeriodicLinearProblem("elasticity", coef, mpc)
    chi = lp.solve()
    ref, chi_r, node = PF.solve_cell(msh, "elasticity", coef)
    assert lp.info == 0 and _rel(lp.effective_tensor, ref) < 1e-10
    for m, f in enumerate(chi):
        d = f.x.array.reshape(-1, 3) - chi_r[m].reshape(-1, 3)[node]
        assert np.abs(d - d.mean(axis=0)).max() < 1e-9 * max(1.0, np.abs(chi_r[m]).max())
