"""The tree route of the mesh family (hommx_plan_create_mesh beyond HOMMX_MESH_MAX_FRONT or with HOMMX_MESH_FLAG_TREE,
csrc/mesh_tree.hip) on an MI355X (-m gpu): accuracy against tests/periodic_fem.py, equivalence with the frontal and the structured
routes, the full C5 size, invariance, failure isolation, samplers, the solver classes end to end, the multi-GPU refusal."""

import ctypes as C
import os

import numpy as np
import pytest

import periodic_fem as PF
from hommx_amd import MicroCellPlan, _lib, fem, hmm, mesh as Mm, workloads as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
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


def _check_correctors(p, chi, msh, ref_chi, node, bs, tol):
    for m in range(chi.shape[0]):
        got = chi[m].reshape(-1, bs)[p.to_periodic]
        want = ref_chi[m].reshape(-1, bs)[node]
        d = got - want
        assert np.abs(d - d.mean(axis=0)).max() < tol * max(1.0, np.abs(want).max())


@pytest.fixture(scope="module")
def cube8():
    return W.jittered_unit_cube(8, 8, 8)


def test_wide_cube_elasticity_against_reference(cube8, rng):
    """Failed with EINVAL before the tree route: jittered 8^3 3D elasticity (frontal width 486)."""
    p = MicroCellPlan.from_mesh(cube8, "elasticity")
    assert p.kernel == "mesh_multifrontal" and p.front_width == 0 and p.flops_per_solve > 0
    coef = _coef("elasticity", 3, cube8.num_cells, rng, nc=3)
    A, chi, info = p.solve(coef, return_info=True, return_correctors=True)
    assert np.all(info == 0)
    for c in range(3):
        ref, ref_chi, node = PF.solve_cell(cube8, "elasticity", coef[c])
        assert _rel(A[c], ref) < 1e-10
        _check_correctors(p, chi[c], cube8, ref_chi, node, 3, 1e-9)
    with pytest.raises(_lib.HommxLibraryError, match="HOMMX_MESH_MAX_FRONT"):
        MicroCellPlan.from_mesh(cube8, "elasticity", route="front")


@pytest.mark.parametrize("case", ["voigt_strat_6", "poisson_matrix_12", "elasticity_2d_60x52"])
def test_other_kinds_against_reference(case, rng):
    if case == "voigt_strat_6":
        msh, kind, dim, M = W.jittered_unit_cube(6, 6, 6, seed=4), "elasticity_voigt", 3, _M(3, 2, rng)
    elif case == "poisson_matrix_12":
        msh, kind, dim, M = W.jittered_unit_cube(12, 12, 12, seed=5), "poisson_matrix", 3, None
    else:
        msh, kind, dim, M = W.jittered_unit_square(60, 52, seed=6), "elasticity", 2, None
    p = MicroCellPlan.from_mesh(msh, kind)
    assert p.kernel == "mesh_multifrontal"
    coef = _coef(kind, dim, msh.num_cells, rng, nc=2)
    A, info = p.solve(coef, M, return_info=True)
    assert np.all(info == 0)
    for c in range(2):
        ref = PF.solve_cell(msh, kind, coef[c], None if M is None else M[c])[0]
        assert _rel(A[c], ref) < 1e-10


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_tree_matches_frontal_on_narrow_meshes(kind, dim, rng):
    msh = W.jittered_unit_square(9, 11, seed=3) if dim == 2 else W.jittered_unit_cube(3, 3, 4, seed=2)
    f = MicroCellPlan.from_mesh(msh, kind)
    t = MicroCellPlan.from_mesh(msh, kind, route="tree")
    assert f.kernel == "mesh_front" and t.kernel == "mesh_multifrontal"
    coef = _coef(kind, dim, msh.num_cells, rng, nc=5)
    for M in (None, _M(dim, 5, rng)):
        At, it = t.solve(coef, M, return_info=True)
        assert np.all(it == 0)
        assert _rel(At, f.solve(coef, M)) < 1e-11
    bs = 1 if kind.startswith("poisson") else dim
    Af, cf = f.solve(coef[:2], return_correctors=True)
    At, ct = t.solve(coef[:2], return_correctors=True)
    for c in range(2):
        for m in range(ct.shape[1]):
            d = (ct[c, m] - cf[c, m]).reshape(-1, bs)
            assert np.abs(d - d.mean(axis=0)).max() < 1e-9 * max(1.0, np.abs(cf[c, m]).max())


@pytest.mark.parametrize("dim,n,kind", [(3, 8, "elasticity"), (2, 100, "poisson")])
def test_structured_mesh_through_the_tree_matches_structured_route(dim, n, kind, rng):
    msh = Mm.create_unit_cube(n, n, n) if dim == 3 else Mm.create_unit_square(n, n)
    p = MicroCellPlan.from_mesh(msh, kind, route="tree")
    q = MicroCellPlan(dim, n, kind)
    assert p.kernel == "mesh_multifrontal"
    coef = _coef(kind, dim, msh.num_cells, rng, nc=4)
    for M in (None, _M(dim, 4, rng)):
        assert _rel(p.solve(coef, M), q.solve(coef, M)) < 1e-11


def test_full_size_c5_golden_cells():
    g = np.load(os.path.join(GOLDEN, "fullsize_c5_n16_strat.npz"))
    msh = Mm.create_unit_cube(16, 16, 16)
    p = MicroCellPlan.from_mesh(msh, "elasticity", route="tree")
    mask = np.unpackbits(g["mask_bits"])[:msh.num_cells].astype(bool)
    coef = np.where(mask[None, :, None], g["values"][:, None, 1, :], g["values"][:, None, 0, :])
    A, info = p.solve(coef, g["M"], return_info=True)
    assert np.all(info == 0)
    assert _rel(A, g["A_eff"]) < 1e-7
    A2 = p.solve_two_phase(mask, g["values"], g["M"])
    assert np.array_equal(A2, A)


def test_full_size_jittered_batch(rng):
    msh = W.jittered_unit_cube(16, 16, 16)
    p = MicroCellPlan.from_mesh(msh, "elasticity")
    assert p.kernel == "mesh_multifrontal"
    nc = 256
    lam = np.where(rng.random((nc, msh.num_cells)) < 0.3, 10.0, 1.0) * rng.uniform(0.8, 1.2, (nc, 1))
    mu = lam * 0.5
    coef = np.stack([lam, mu], -1)
    A, info = p.solve(coef, return_info=True)
    assert np.all(info == 0)
    assert np.abs(A - np.swapaxes(A, 1, 2)).max() < 1e-10 * np.abs(A).max()
    assert np.all(np.linalg.eigvalsh(A) > 0)
    # Voigt (volume mean of C) and Reuss (inverse volume mean of C^-1) bounds, in the Voigt basis of the library's tensors
    vol = msh.cell_volumes()
    Cel = np.stack([PF.material_tensor("elasticity", coef[c], 3) for c in (0, nc - 1)])  # [2, e, 3, 3, 3, 3]
    E = PF.unit_strains(3)
    Cv = np.einsum("mij,ceijkl,nkl->cemn", E, Cel, E)
    voigt = np.einsum("e,cemn->cmn", vol, Cv)
    reuss = np.linalg.inv(np.einsum("e,cemn->cmn", vol, np.linalg.inv(Cv)))
    for k, c in enumerate((0, nc - 1)):
        assert np.linalg.eigvalsh(voigt[k] - A[c]).min() > -1e-9 * np.abs(voigt[k]).max()
        assert np.linalg.eigvalsh(A[c] - reuss[k]).min() > -1e-9 * np.abs(voigt[k]).max()


def test_invariance_position_batch_and_renumbering(cube8, rng):
    p = MicroCellPlan.from_mesh(cube8, "elasticity")
    nc = 40
    coef = _coef("elasticity", 3, cube8.num_cells, rng, nc=nc)
    A = p.solve(coef)
    one = p.solve(coef[17:18])
    assert np.array_equal(one[0], A[17])
    shuffled = np.roll(coef, 5, axis=0)
    assert np.array_equal(p.solve(shuffled)[22], A[17])
    big = np.concatenate([coef] * 8)  # 320 cells: several pieces and streams
    Ab = p.solve(big)
    assert np.array_equal(Ab[17 + 5 * nc], A[17]) and np.array_equal(Ab[-1], A[-1])
    # element and node renumbering: same tensors to rounding
    perm = rng.permutation(cube8.num_cells)
    vperm = rng.permutation(cube8.geometry.x.shape[0])
    inv = np.argsort(vperm)
    msh2 = Mm.create_mesh(inv[np.asarray(cube8.cells)[perm]], cube8.geometry.x[vperm])
    p2 = MicroCellPlan.from_mesh(msh2, "elasticity")
    assert _rel(p2.solve(coef[:4][:, perm]), A[:4]) < 1e-11


def test_bad_cells_flagged_neighbours_unaffected(cube8, rng):
    p = MicroCellPlan.from_mesh(cube8, "elasticity")
    coef = _coef("elasticity", 3, cube8.num_cells, rng, nc=6)
    A0 = p.solve(coef)
    bad = coef.copy()
    bad[1, 10, 1] = np.nan
    bad[4, :, 1] = -1.0
    A, info = p.solve(bad, return_info=True)
    assert info[1] != 0 and info[4] != 0
    for c in (0, 2, 3, 5):
        assert info[c] == 0 and np.array_equal(A[c], A0[c])


def test_samplers_match_host_stream(cube8, rng):
    p = MicroCellPlan.from_mesh(cube8, "elasticity")
    mask = rng.random(cube8.num_cells) < 0.4
    values = rng.uniform(0.5, 3.0, (5, 2, 2))
    M = _M(3, 5, rng)
    coef = np.where(mask[None, :, None], values[:, None, 1, :], values[:, None, 0, :])
    assert _rel(p.solve_two_phase(mask, values, M), p.solve(coef, M)) < 1e-13
    q = MicroCellPlan.from_mesh(W.jittered_unit_square(60, 52, seed=6), "poisson", route="tree")
    assert q.kernel == "mesh_multifrontal"
    table = rng.uniform(0.5, 2.0, q.n_el)
    params = rng.uniform(0.5, 2.0, (4, 2))
    ref = q.solve(params[:, :1] + params[:, 1:] * table[None, :])
    assert _rel(q.solve_separable("affine", table, None, params), ref) < 1e-13


def _twin_with_reference(h):
    def eff(cells):
        coef, kind = h._element_means(cells)
        M = h._stratification(cells)
        out = np.stack([PF.solve_cell(h._cell_mesh, kind, coef[i], None if M is None else M[i])[0] for i in range(len(cells))])
        return out, np.zeros(len(cells), np.int32)

    h._effective_tensors = eff
    return h


def test_elasticity_stratified_hmm_tree_micro(cube8):
    def A(x, y):
        return hmm.Lame(1.0 + 0.0 * y[0], np.where(np.cos(2 * np.pi * y[2]) > 0, 8.0, 0.5))

    def Dt(x):
        return np.array([[1.0, 0.0, 0.0], [0.2 * np.cos(x[0]), 1.0, 0.0], [0.0, 0.0, 1.0]])

    def mk():
        msh = Mm.create_box([(0, 0, 0), (1.0, 0.5, 0.5)], (2, 1, 1))
        h = hmm.LinearElasticityStratifiedHMM(msh, A, lambda x: np.array([0.0, 0.0, -0.01]), cube8, 2.0**-4, Dt)
        V = h.function_space
        clamp = fem.locate_dofs_topological(V, 2, fem.locate_entities_boundary(msh, 2, lambda x: np.isclose(x[0], 0)))
        h.set_boundary_conditions(fem.dirichletbc(np.zeros(3), clamp, V))
        return h

    h = mk()
    u = h.solve()
    assert np.all(h.cell_info == 0)
    ur = _twin_with_reference(mk()).solve()
    assert np.abs(u.x.array - ur.x.array).max() < 1e-10 * np.abs(ur.x.array).max()


def test_periodic_linear_problem_on_wide_mesh(rng):
    from hommx_amd.cell_problem import PeriodicLinearProblem, create_periodic_boundary_conditions

    msh = W.jittered_unit_square(60, 52, seed=6)
    V = fem.FunctionSpace(msh, 2)
    mpc = create_periodic_boundary_conditions(V)
    coef = _coef("elasticity", 2, msh.num_cells, rng)
    lp = PeriodicLinearProblem("elasticity", coef, mpc)
    assert lp._plan.kernel == "mesh_multifrontal"
    chi = lp.solve()
    ref, chi_r, node = PF.solve_cell(msh, "elasticity", coef)
    assert lp.info == 0 and _rel(lp.effective_tensor, ref) < 1e-10
    for m, f in enumerate(chi):
        d = f.x.array.reshape(-1, 2) - chi_r[m].reshape(-1, 2)[node]
        assert np.abs(d - d.mean(axis=0)).max() < 1e-9 * max(1.0, np.abs(chi_r[m]).max())


def test_multi_refuses_tree_plans():
    lib = _lib.load()
    comm = C.c_void_p()
    _lib.check(lib.hommx_comm_init_all(C.byref(comm), 1, None), "hommx_comm_init_all")
    try:
        p = MicroCellPlan.from_mesh(W.jittered_unit_square(6, 6), "poisson", route="tree")
        assert p.kernel == "mesh_multifrontal"
        plans = (C.c_void_p * 1)(p._h.value)
        coef = np.ones((2, p.n_el))
        out = np.zeros((2, 2, 2))
        info = np.zeros(2, np.int32)
        rc = lib.hommx_solve_batch_multi(comm, plans, 2, coef.ctypes.data, None, out.ctypes.data, info.ctypes.data)
        assert rc == -1 and "mesh plan" in _lib.last_error()
    finally:
        lib.hommx_comm_destroy(comm)
