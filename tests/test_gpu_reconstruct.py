"""HMM reconstruction on an MI355X (-m gpu): hommx_reconstruct_batch[_device] on every route against the NumPy reference
(tests/recon_ref.py), its exact identities, a closed form, invariance (batch position, chunking, fields, device entry), a failing cell,
the production C5 size and the solver classes end to end."""

import os

import numpy as np
import pytest

import recon_ref as R
from hommx_amd import MicroCellPlan, fem, hmm, mesh as Mm, workloads as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
STAT_NAMES = ("mean_strain", "mean_flux", "energy", "max_flux", "argmax_element")


def _t(kind, dim):
    return dim if kind.startswith("poisson") else dim * (dim + 1) // 2


def _batch(kind, dim, n_el, nc, rng, strat):
    coef = np.stack([R.random_coef(kind, dim, n_el, rng) for _ in range(nc)])
    M = np.stack([R.random_M(dim, rng) for _ in range(nc)]) if strat else None
    xi = rng.standard_normal((nc, _t(kind, dim)))
    return coef, M, xi


def _check_against(r, refs, fields=True):
    for k, ref in enumerate(refs):
        if fields:
            for got, want in ((r.strain[k], ref["s"]), (r.flux[k], ref["q"])):
                assert np.abs(got - want).max() < 1e-9 * np.abs(want).max()
        fs = np.abs(ref["q"]).max()
        assert np.abs(r.mean_strain[k] - ref["mean_strain"]).max() < 1e-10 * np.abs(ref["s"]).max()
        assert np.abs(r.mean_flux[k] - ref["mean_flux"]).max() < 1e-10 * fs
        assert abs(r.energy[k] - ref["energy"]) < 1e-10 * abs(ref["energy"])
        assert abs(r.max_flux[k] - ref["max_flux"]) < 1e-10 * ref["max_flux"]


def _check_identities(r, A):
    """mean strain = xi, mean flux = A xi, energy = xi . A xi, with A from the plan's own tensor route."""
    for k in range(len(r.xi)):
        xi = r.xi[k]
        Ax = A[k] @ xi
        assert np.abs(r.mean_strain[k] - xi).max() < 1e-12 * np.abs(xi).max()
        assert np.abs(r.mean_flux[k] - Ax).max() < 1e-10 * np.abs(A[k]).max() * np.abs(xi).max()
        assert abs(r.energy[k] - xi @ Ax) < 1e-10 * abs(xi @ Ax)


ROUTES = [  # (dim, n, kind, expected kernel of the plan's tensor route)
    (2, 8, "poisson", "fused2d"),
    (2, 32, "poisson", "fused2d"),
    (2, 10, "elasticity", "small_wave"),
    (3, 6, "poisson", "small_wave"),
    (3, 8, "poisson", "small_fused"),
    (2, 64, "poisson", "multifrontal"),
    (3, 5, "elasticity", "multifrontal"),
    (2, 8, "poisson_matrix", None),
    (3, 4, "elasticity_voigt", None),
]


@pytest.mark.parametrize("dim,n,kind,route", ROUTES)
@pytest.mark.parametrize("strat", [False, True])
def test_every_route_matches_reference(dim, n, kind, route, strat):
    rng = np.random.default_rng(100 * dim + n + 7 * strat)
    p = MicroCellPlan(dim, n, kind)
    if route:
        assert p.kernel == route
    coef, M, xi = _batch(kind, dim, p.n_el, 3, rng, strat)
    r = p.reconstruct(coef, xi, M, fields=True)
    assert not r.info.any()
    refs = [R.structured(kind, dim, n, coef[k], None if M is None else M[k], xi[k]) for k in range(3)]
    _check_against(r, refs)
    A = p.solve(coef, M)
    _check_identities(r, A)
    assert np.abs(r.A_eff - A).max() < 1e-10 * np.abs(A).max()
    nrm = np.linalg.norm(r.flux, axis=2) if kind.startswith("poisson") else None
    if nrm is not None:
        assert np.array_equal(r.argmax_element, np.argmax(nrm, axis=1)) or np.allclose(nrm[np.arange(3), r.argmax_element], nrm.max(axis=1))


def _mesh_plan_pair(msh, kind):
    return MicroCellPlan.from_mesh(msh, kind, route="front"), MicroCellPlan.from_mesh(msh, kind, route="tree")


@pytest.mark.parametrize("dim,kind", [(2, "poisson"), (2, "elasticity"), (3, "poisson_matrix"), (3, "elasticity_voigt")])
def test_mesh_routes_match_reference(dim, kind):
    rng = np.random.default_rng(5 + dim)
    msh = W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)
    front, tree = _mesh_plan_pair(msh, kind)
    assert front.kernel == "mesh_front" and tree.kernel == "mesh_multifrontal"
    coef, M, xi = _batch(kind, dim, front.n_el, 3, rng, True)
    rf = front.reconstruct(coef, xi, M, fields=True)
    rt = tree.reconstruct(coef, xi, M, fields=True)
    refs = [R.on_mesh(msh, kind, coef[k], M[k], xi[k]) for k in range(3)]
    _check_against(rf, refs)
    _check_against(rt, refs)
    for a, b in ((rf.strain, rt.strain), (rf.flux, rt.flux)):
        assert np.abs(a - b).max() < 1e-10 * np.abs(a).max()
    _check_identities(rf, front.solve(coef, M))


def test_mesh_plan_of_structured_grid_matches_structured_plan():
    rng = np.random.default_rng(17)
    msh = Mm.create_unit_square(16, 16)
    s = MicroCellPlan(2, 16, "elasticity")
    m = MicroCellPlan.from_mesh(msh, "elasticity")
    coef, M, xi = _batch("elasticity", 2, s.n_el, 3, rng, True)
    a = s.reconstruct(coef, xi, M, fields=True)
    b = m.reconstruct(coef, xi, M, fields=True)
    for x, y in ((a.strain, b.strain), (a.flux, b.flux)):
        assert np.abs(x - y).max() < 1e-10 * np.abs(x).max()


def test_laminate_closed_form():
    """C1 laminate (layers normal to y0, conforming to the grid): the normal flux is A_H[0, 0] xi_0 in every element and the tangential
    gradient is xi_1 everywhere.  The tangential corrector is zero up to the rounding of the corrector solve (condition about contrast x n^2
    = 2.5e4), which its gradient carries: that check holds to 1e-11."""
    msh, coef, _ = W.c1_laminate(nx=2, n=16)
    AH = W.c1_exact(msh)
    p = MicroCellPlan(2, 16, "poisson")
    rng = np.random.default_rng(2)
    xi = rng.standard_normal((coef.shape[0], 2))
    r = p.reconstruct(coef, xi, fields=True)
    for k in range(coef.shape[0]):
        q0 = AH[k, 0, 0] * xi[k, 0]
        assert np.abs(r.flux[k, :, 0] - q0).max() < 1e-12 * max(abs(q0), np.abs(AH[k]).max() * np.abs(xi[k]).max())
        assert np.abs(r.strain[k, :, 1] - xi[k, 1]).max() < 1e-11 * np.abs(xi[k]).max()


def _stats(r):
    return np.concatenate([r.mean_strain, r.mean_flux, r.energy[:, None], r.max_flux[:, None], r.argmax_element[:, None]], axis=1)


@pytest.mark.parametrize("dim,n,kind", [(2, 16, "poisson"), (3, 5, "elasticity"), (2, 10, "elasticity")])
def test_stats_independent_of_fields_and_chunking(dim, n, kind, monkeypatch):
    rng = np.random.default_rng(23)
    p = MicroCellPlan(dim, n, kind)
    nc = 130 if dim == 3 else 600
    coef, M, xi = _batch(kind, dim, p.n_el, nc, rng, True)
    a = p.reconstruct(coef, xi, M)
    b = p.reconstruct(coef, xi, M, fields=True)
    assert np.array_equal(_stats(a), _stats(b))
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")  # read when the plan is created: many chunks
    q = MicroCellPlan(dim, n, kind)
    c = q.reconstruct(coef, xi, M, fields=True)
    assert np.array_equal(_stats(a), _stats(c))
    assert np.array_equal(b.strain, c.strain) and np.array_equal(b.flux, c.flux)


@pytest.mark.parametrize("case", ["fused2d", "small_wave", "multifrontal", "mesh_front", "mesh_tree"])
def test_batch_position(case):
    rng = np.random.default_rng(31)
    if case.startswith("mesh"):
        msh = W.jittered_unit_square(8, 8)
        p = MicroCellPlan.from_mesh(msh, "poisson", route=case[5:])
        kind, dim = "poisson", 2
    else:
        dim, n, kind = {"fused2d": (2, 32, "poisson"), "small_wave": (2, 10, "elasticity"), "multifrontal": (3, 5, "elasticity")}[case]
        p = MicroCellPlan(dim, n, kind)
        assert p.kernel == case
    coef, M, xi = _batch(kind, dim, p.n_el, 64, rng, True)
    big = _stats(p.reconstruct(coef, xi, M))
    for k in (0, 37, 63):
        one = _stats(p.reconstruct(coef[k:k + 1], xi[k:k + 1], M[k:k + 1]))[0]
        if case in ("multifrontal", "mesh_front", "mesh_tree"):
            assert np.array_equal(one, big[k]), case
        else:
            assert np.abs(one[:-1] - big[k][:-1]).max() <= 1e-13 * np.abs(big[k][:-1]).max()


def test_device_entry_equals_host_entry():
    import torch

    rng = np.random.default_rng(41)
    p = MicroCellPlan(3, 5, "elasticity")
    nc, t = 5, 6
    coef, M, xi = _batch("elasticity", 3, p.n_el, nc, rng, True)
    host = p.reconstruct(coef, xi, M, fields=True)
    dev = torch.device("cuda", p.device)
    dc, dM, dx = (torch.from_numpy(a).to(dev) for a in (coef, M, xi))
    stats = torch.empty((nc, 2 * t + 3), dtype=torch.float64, device=dev)
    s = torch.empty((nc, p.n_el, t), dtype=torch.float64, device=dev)
    q = torch.empty_like(s)
    A = torch.empty((nc, t, t), dtype=torch.float64, device=dev)
    info = torch.full((nc,), -7, dtype=torch.int32, device=dev)
    p.reconstruct_device(nc, dc.data_ptr(), dM.data_ptr(), dx.data_ptr(), stats.data_ptr(), s.data_ptr(), q.data_ptr(), A.data_ptr(),
                         info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(stats.cpu().numpy(), _stats(host))
    assert np.array_equal(s.cpu().numpy(), host.strain) and np.array_equal(q.cpu().numpy(), host.flux)
    assert np.array_equal(A.cpu().numpy(), host.A_eff) and np.array_equal(info.cpu().numpy(), host.info)


def test_bad_cell_is_isolated():
    rng = np.random.default_rng(43)
    p = MicroCellPlan(3, 5, "elasticity")
    coef, M, xi = _batch("elasticity", 3, p.n_el, 6, rng, True)
    good = p.reconstruct(coef, xi, M)
    bad_coef = coef.copy()
    bad_coef[2, 17, 1] = np.nan
    bad = p.reconstruct(bad_coef, xi, M)
    assert bad.info[2] != 0 and not np.delete(bad.info, 2).any()
    assert np.array_equal(np.delete(_stats(bad), 2, axis=0), np.delete(_stats(good), 2, axis=0))
    keep = [0, 1, 3, 4, 5]
    without = p.reconstruct(coef[keep], xi[keep], M[keep])  # the batch without the cell (this route is position-independent)
    assert np.array_equal(np.delete(_stats(bad), 2, axis=0), _stats(without))


def test_production_c5_cells():
    g = np.load(os.path.join(GOLDEN, "fullsize_c5_n16_strat.npz"))
    mask = np.unpackbits(g["mask_bits"])[:24576].astype(bool)
    coef = g["values"][:, mask.astype(int), :]  # [3, n_el, (lambda, mu)]
    M, A = g["M"], g["A_eff"]
    p = MicroCellPlan(3, 16, "elasticity")
    rng = np.random.default_rng(53)
    for xi0 in list(np.eye(6)) + [rng.standard_normal(6)]:
        xi = np.repeat(xi0[None], 3, axis=0)
        r = p.reconstruct(coef, xi, M)
        assert not r.info.any()
        for k in range(3):
            Ax = A[k] @ xi0
            assert np.abs(r.mean_flux[k] - Ax).max() < 1e-7 * np.abs(A[k]).max() * np.abs(xi0).max()
            assert np.abs(r.mean_strain[k] - xi0).max() < 1e-10 * np.abs(xi0).max()
            assert r.max_flux[k] >= np.linalg.norm(Ax) * (1 - 1e-9) / np.sqrt(2) and 0 <= r.argmax_element[k] < p.n_el


def test_poisson_hmm_end_to_end():
    msh = Mm.create_unit_square(16, 16)
    A = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.001 * (1.0 + 9.0 * x[0]), lambda x: 0.1 + 0.0 * x[0])
    h = hmm.PoissonHMM(msh, A, lambda x: 1.0 + x[0], Mm.create_unit_square(32, 32), 0.01)
    V = h.function_space
    h.set_boundary_conditions(fem.dirichletbc(0.0, fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[1], 1)), V))
    u = h.solve()
    r = h.reconstruct()
    assert not r.info.any()
    macro = u.x.array @ (h._A @ u.x.array)
    assert abs(msh.cell_volumes() @ r.energy - macro) < 1e-10 * abs(macro)
    two = h.reconstruct(cells=[3, 200], fields=True)
    coef, _ = h._element_means(np.array([3, 200]))
    direct = h._plan.reconstruct(coef, r.xi[[3, 200]], None, fields=True)
    assert np.array_equal(two.flux, direct.flux) and np.array_equal(two.strain, direct.strain)
    assert np.array_equal(two.energy, r.energy[[3, 200]])


def test_elasticity_stratified_hmm_end_to_end():
    msh = Mm.create_box([(0.0, 0.0, 0.0), (1.0, 0.4, 0.4)], (4, 2, 2))

    def A(x, y):
        return hmm.Lame(1.0, np.where(W.wrapped_disc(y[1], y[2]), 100.0, 0.01))

    def Dt(x):
        g = 0.5 * np.pi * x[1]
        return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-0.3 * np.sin(g), 0.1 * np.cos(g), 1.0]])

    h = hmm.LinearElasticityStratifiedHMM(msh, A, lambda x: np.array([0.0, 0.0, -0.01]), Mm.create_unit_cube(6, 6, 6), 0.05, Dt)
    V = h.function_space
    clamp = fem.locate_dofs_topological(V, 2, fem.locate_entities_boundary(msh, 2, lambda x: np.isclose(x[0], 0)))
    h.set_boundary_conditions(fem.dirichletbc(np.zeros(3), clamp, V))
    u = h.solve()
    r = h.reconstruct()
    assert not r.info.any()
    macro = u.x.array @ (h._A @ u.x.array)
    assert abs(msh.cell_volumes() @ r.energy - macro) < 1e-10 * abs(macro)
    two = h.reconstruct(cells=[0, 7], fields=True)
    coef, _ = h._element_means(np.array([0, 7]))
    direct = h._plan.reconstruct(coef, r.xi[[0, 7]], h._stratification(np.array([0, 7])), fields=True)
    assert np.array_equal(two.flux, direct.flux) and np.array_equal(two.strain, direct.strain)
