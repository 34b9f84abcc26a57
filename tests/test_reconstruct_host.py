"""HMM reconstruction on the CPU: the NumPy reference's identities, the solver classes' reconstruct() on an oracle-backed stub plan, and
the C ABI's argument checks (no GPU needed)."""

import ctypes
import os

import numpy as np
import pytest

import recon_ref as R
from hommx_amd import fem, hmm, mesh
from hommx_amd.batch import Reconstruction
from oracle import hommx_oracle as O

KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,n", [(2, 5), (3, 3)])
@pytest.mark.parametrize("strat", [False, True])
def test_reference_identities(kind, dim, n, strat):
    """mean strain = xi (periodic correctors have mean-free gradients), mean flux = A xi (Schur form), energy = xi . A xi (Hill-Mandel)."""
    rng = np.random.default_rng(7 + dim + 10 * KINDS.index(kind) + 100 * strat)
    n_el = (2 if dim == 2 else 6) * n**dim
    coef = R.random_coef(kind, dim, n_el, rng)
    M = R.random_M(dim, rng) if strat else None
    t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
    xi = rng.standard_normal(t)
    r = R.structured(kind, dim, n, coef, M, xi)
    A = r["A"]
    scale = np.abs(A).max() * np.abs(xi).max()
    assert np.abs(r["mean_strain"] - xi).max() < 1e-12 * np.abs(xi).max()
    assert np.abs(r["mean_flux"] - A @ xi).max() < 1e-12 * scale
    assert abs(r["energy"] - xi @ A @ xi) < 1e-12 * scale * np.abs(xi).max() * t
    assert r["max_flux"] == pytest.approx(np.max(np.linalg.norm(r["q"], axis=1)) if kind.startswith("poisson") else r["max_flux"])


def test_reference_mesh_matches_structured():
    rng = np.random.default_rng(3)
    coef = R.random_coef("elasticity", 2, 2 * 36, rng)
    xi = rng.standard_normal(3)
    a = R.structured("elasticity", 2, 6, coef, None, xi)
    b = R.on_mesh(mesh.create_unit_square(6, 6), "elasticity", coef, None, xi)
    assert np.abs(a["s"] - b["s"]).max() < 1e-10 * np.abs(a["s"]).max()
    assert np.abs(a["q"] - b["q"]).max() < 1e-10 * np.abs(a["q"]).max()


# -- solver classes on an oracle-backed stub plan (the pattern of tests/test_hmm_host.py) ------------------------------------------------
class ReconOraclePlan:
    """Answers solve() / reconstruct() with the CPU reference; records the batch sizes it was given."""

    def __init__(self, dim, n, kind):
        self.dim, self.n, self.kind = dim, n, kind
        self.t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
        self.batches = []

    def solve(self, coef, M=None, return_info=False):
        out = np.stack([R.structured(self.kind, self.dim, self.n, coef[k], None if M is None else M[k], np.zeros(self.t))["A"]
                        for k in range(len(coef))])
        info = np.zeros(len(coef), np.int32)
        return (out, info) if return_info else out

    def reconstruct(self, coef, xi, M=None, fields=False):
        self.batches.append(len(coef))
        rs = [R.structured(self.kind, self.dim, self.n, coef[k], None if M is None else M[k], xi[k]) for k in range(len(coef))]
        t = self.t
        stats = np.array([np.r_[r["mean_strain"], r["mean_flux"], r["energy"], r["max_flux"], r["argmax_element"]] for r in rs]).reshape(-1, 2 * t + 3)
        A = np.stack([r["A"] for r in rs])
        s = np.stack([r["s"] for r in rs]) if fields else None
        q = np.stack([r["q"] for r in rs]) if fields else None
        return Reconstruction.from_stats(np.asarray(xi), stats, A, np.zeros(len(coef), np.int32), s, q)


def with_stub(h):
    kind = "poisson" if h._kind == "poisson" else "elasticity"
    h._plan = ReconOraclePlan(h._tdim, h._n_micro, kind)
    return h


def poisson_solver(nx=3, n=4):
    A = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * x[0]) + 0.9 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1])
    return with_stub(hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: 1.0 + x[0], mesh.create_unit_square(n, n), 0.01,
                                    quadrature_degree=3))


def elasticity_solver(nx=2, n=3):
    lam = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0])
    mu = lambda x, y: 0.6 + 0.3 * np.cos(2 * np.pi * y[1]) + 0.1 * x[0]
    A = lambda x, y: hmm.Lame(lam(x, y), mu(x, y))
    msh = mesh.create_unit_cube(nx, nx, nx)
    h = hmm.LinearElasticityStratifiedHMM(msh, A, lambda x: np.array([0.0, 0.0, -1.0]), mesh.create_unit_cube(n, n, n), 0.01,
                                          lambda x: np.array([[1.0, 0.1, 0.0], [0.0, 1.0, 0.2], [0.0, 0.0, 1.0]]), quadrature_degree=0)
    return with_stub(h)


def test_affine_field_gives_constant_xi_poisson():
    h = poisson_solver()
    a = np.array([0.7, -1.3])
    u = h.function_space.tabulate_dof_coordinates()[:, :2] @ a
    r = h.reconstruct(u)
    assert np.abs(r.xi - a).max() < 1e-12
    assert np.abs(r.mean_strain - a).max() < 1e-12
    assert np.array_equal(r.cells, np.arange(h._msh.num_cells))


def test_affine_field_gives_constant_xi_elasticity():
    h = elasticity_solver()
    G = np.array([[0.3, -0.2, 0.5], [0.1, 0.4, -0.6], [0.7, 0.2, -0.1]])  # u = G x
    x = h.function_space.tabulate_dof_coordinates()[:, :3]
    u = (x @ G.T).ravel()
    e = 0.5 * (G + G.T)
    want = np.array([e[0, 0], e[1, 1], e[2, 2], 2 * e[0, 1], 2 * e[0, 2], 2 * e[1, 2]])
    r = h.reconstruct(u, cells=[0, 5, 11])
    assert np.abs(r.xi - want).max() < 1e-12


@pytest.mark.parametrize("make", [poisson_solver, elasticity_solver])
def test_energy_sums_to_macro_energy(make):
    h = make()
    V = h.function_space
    bnd = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1))
    h.set_boundary_conditions(fem.dirichletbc(0.0 if h._kind == "poisson" else np.zeros(3), bnd, V))
    u = h.solve()
    r = h.reconstruct()
    vol = h._msh.cell_volumes()
    macro = u.x.array @ (h._A @ u.x.array)
    assert abs(vol @ r.energy - macro) < 1e-12 * abs(macro)
    assert np.abs(r.mean_flux - np.einsum("cmn,cn->cm", h.effective_tensors, r.xi)).max() < 1e-10 * np.abs(r.mean_flux).max()


def test_subset_and_chunking_give_the_same_numbers():
    h = poisson_solver()
    h.solve()
    full = h.reconstruct(fields=True)
    sub = h.reconstruct(cells=[4, 1, 9], fields=True)
    small = h.reconstruct(chunk_cells=2)
    assert h._plan.batches[-1] == 2 and max(h._plan.batches[-9:]) == 2
    for name in ("xi", "mean_strain", "mean_flux", "energy", "max_flux", "argmax_element"):
        assert np.array_equal(getattr(sub, name), getattr(full, name)[[4, 1, 9]]), name
        assert np.array_equal(getattr(small, name), getattr(full, name)), name
    assert np.array_equal(sub.flux, full.flux[[4, 1, 9]])
    assert small.strain is None


def test_reconstruct_before_solve_raises():
    h = poisson_solver()
    with pytest.raises(RuntimeError, match="solve"):
        h.reconstruct()


# -- C ABI argument checks ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from hommx_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_abi_argument_checks(lib):
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert lib.hommx_reconstruct_batch(None, 1, p, None, p, p, None, None, None, None) == -1
    assert "null plan" in lib.hommx_last_error().decode()
    assert lib.hommx_reconstruct_batch_device(None, 1, p, None, p, p, None, None, None, None, None) == -1
    # a plan-shaped pointer is never dereferenced before the pointer checks: null xi / stats fail first
    fake = ctypes.create_string_buffer(4096)
    for args in ((p, None, None, p), (p, None, p, None), (None, None, p, p)):
        assert lib.hommx_reconstruct_batch(ctypes.addressof(fake), 1, *args, None, None, None, None) == -1
        assert "null coef / xi / stats" in lib.hommx_last_error().decode()
    assert lib.hommx_reconstruct_batch(None, 0, None, None, None, None, None, None, None, None) == -1  # null plan, even when empty
    assert lib.hommx_reconstruct_batch(ctypes.addressof(fake), -1, p, None, p, p, None, None, None, None) == -1


def test_energy_density_reference_matches_oracle_energy_form():
    """The reference's per-element energy sums to the oracle's energy-form tensor (a check of the reference itself)."""
    rng = np.random.default_rng(11)
    coef = R.random_coef("elasticity", 3, 6 * 27, rng)
    cp = O.build_cell_problem("elasticity", 3, 3, coef)
    A = O.effective_tensor(cp, form="energy")
    for m in range(6):
        xi = np.eye(6)[m]
        assert R.structured("elasticity", 3, 3, coef, None, xi)["energy"] == pytest.approx(A[m, m], rel=1e-11)
