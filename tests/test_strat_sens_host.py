"""Derivatives of A_H with respect to the stratification M on the CPU: the two forms of the NumPy reference (tests/strat_sens_ref.py)
against each other, against central differences of the reference's own A_H, the zero-homogeneity identity and the laminate closed form;
the exports and the argument checks of hommx_stratification_sensitivity_source[_device] (they run before any device is touched); and
BaseHMM.stratification_derivatives / stratification_energy_derivatives on a stub plan that answers from the reference (no GPU needed)."""

import ctypes
import functools
import os

import numpy as np
import pytest

import recon_ref as R
import strat_sens_ref as S
from hommx_amd import _lib, hmm, mesh, workloads as W
from hommx_amd.batch import CoefStream, StratSensitivities
from test_reconstruct_host import ReconOraclePlan

KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")
JITTERED = [(kind, dim, None) for dim in (2, 3) for kind in KINDS]
STRUCTURED = [(kind, dim, n) for dim in (2, 3) for kind in KINDS for n in (3, 4, 5)]
CASES = STRUCTURED + JITTERED


@functools.lru_cache(maxsize=None)
def _mesh(dim):
    return W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)


@functools.lru_cache(maxsize=None)
def _case(case):
    """A random coefficient of contrast 1e2 with a random M: the reference cell and its derivative by the moment form."""
    kind, dim, n = case
    rng = np.random.default_rng(CASES.index(case) + 4120)
    n_el = (2 if dim == 2 else 6) * n**dim if n else len(_mesh(dim).cells)
    coef, M = R.random_coef(kind, dim, n_el, rng), R.random_M(dim, rng)
    sc = S.structured(kind, dim, n, coef, M) if n else S.on_mesh(_mesh(dim), kind, coef, M)
    return sc, S.dA_dM(sc)


def _id(case):
    return f"{case[0]}-{case[1]}d-" + (f"n{case[2]}" if case[2] else "jittered")


@pytest.mark.parametrize("case", JITTERED, ids=_id)
def test_moment_form_equals_operator_form(case):
    sc, dA = _case(case)
    err = np.abs(dA - S.dA_dM_operator(sc)).max() / np.abs(sc.A).max()
    print(_id(case), "moment form against the operator form", err)
    assert err < 1e-13
    assert np.array_equal(dA, np.swapaxes(dA, 2, 3))
    assert np.abs(dA).max() > 1e-2 * np.abs(sc.A).max()  # not vacuous


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_reference_against_central_differences(case):
    """h = 1e-6 along every unit direction E_ab: the rounding floor eps / h times the conditioning is of order 1e-10 on these cells."""
    sc, dA = _case(case)
    err = np.abs(dA - S.central_difference(sc, 1e-6)).max() / np.abs(sc.A).max()
    print(_id(case), "central differences", err)
    assert err < 1e-8


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_zero_homogeneity(case):
    """A_H is 0-homogeneous in M (scaling M rescales the correctors): sum_ab M_ab dA_dM[a][b] = 0; and the adjoint product pairs."""
    sc, dA = _case(case)
    err = np.abs(np.einsum("ab,abmn->mn", sc.M, dA)).max() / np.abs(sc.A).max()
    print(_id(case), "homogeneity", err)
    assert err < 1e-13
    w = np.random.default_rng(5).standard_normal((sc.t, sc.t))
    g = S.grad_M(sc, w)
    assert np.abs(g - np.einsum("mn,abmn->ab", w, dA)).max() < 1e-13 * np.abs(w).max() * np.abs(dA).max() * sc.t**2


def test_laminate_closed_form():
    rng = np.random.default_rng(6)
    n = 6
    a = rng.uniform(1.0, 5.0, n)
    M = R.random_M(2, rng)
    sc = S.structured("poisson", 2, n, S.laminate_coef(n, a), M)
    A, dA = S.laminate_exact(a, M)
    assert np.abs(sc.A - A).max() < 1e-12 * a.mean()
    err = np.abs(S.dA_dM(sc) - dA).max() / a.mean()
    print("laminate", err)
    assert err < 1e-12
    assert np.abs(dA).max() > 1e-2 * a.mean()


# -- the library ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_library_exports_both_symbols(lib):
    for name in ("hommx_stratification_sensitivity_source", "hommx_stratification_sensitivity_source_device"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    """Every fault is reported on plan-shaped memory whose descriptor alone is read: no device is touched."""
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_stratification_sensitivity_source_device if device_entry else lib.hommx_stratification_sensitivity_source
    tail = (None,) if device_entry else ()

    def call(plan, src, args, n_cells=1):
        rc = fn(plan, n_cells, src, None, None if args is None else ctypes.byref(args), *tail)
        return rc, lib.hommx_last_error().decode()

    fake = ctypes.create_string_buffer(4096)
    ctypes.memmove(fake, ctypes.byref(_lib.PlanDesc(2, 8, _lib.KIND_POISSON_SCALAR, 0, 0)), ctypes.sizeof(_lib.PlanDesc))
    plan = ctypes.addressof(fake)
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    good = _lib.StratSensArgs(dA_dM=p)
    rc, msg = call(None, sampled, good)
    assert rc == -1 and "null plan" in msg
    assert call(None, sampled, good, n_cells=0)[0] == -1  # null plan, even when empty
    assert call(plan, sampled, good, n_cells=-1)[0] == -1
    rc, msg = call(plan, None, good)
    assert rc == -1 and "null source" in msg
    rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=_lib.COEF_TWO_PHASE, mask=p)), good)
    assert rc == -1 and "null mask / values" in msg
    rc, msg = call(plan, sampled, None)
    assert rc == -1 and "null arguments" in msg
    for args in (_lib.StratSensArgs(dA_dM=p, weights=p), _lib.StratSensArgs(grad_M=p)):
        rc, msg = call(plan, sampled, args)
        assert rc == -1 and "weights and grad_M: both or neither" in msg
    rc, msg = call(plan, sampled, _lib.StratSensArgs(A_eff=p))
    assert rc == -1 and "nothing requested" in msg
    assert call(plan, sampled, good, n_cells=0)[0] == 0  # an empty batch


# -- solver classes on a stub plan that answers from the reference ---------------------------------------------------------------------------
class StratOraclePlan(ReconOraclePlan):
    """solve() of the oracle-backed stand-in, and stratification_sensitivities() from tests/strat_sens_ref.py; records what it was given."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.seen = []

    def stratification_sensitivities(self, coef, M=None, weights=None, full=True):
        self.seen.append((coef, M, weights, full))
        assert not isinstance(coef, CoefStream)
        cells = [S.structured(self.kind, self.dim, self.n, coef[k], None if M is None else M[k]) for k in range(len(coef))]
        dA = np.stack([S.dA_dM(c) for c in cells]) if full else None
        g = None if weights is None else np.stack([S.grad_M(c, weights[k]) for k, c in enumerate(cells)])
        return StratSensitivities(dA, g, np.stack([c.A for c in cells]), np.zeros(len(coef), np.int32))


PHI0 = 0.3


def _rotation(phi0):
    """Dtheta^T(x; phi0): a rotation by phi0 + x0."""

    def f(x):
        a = phi0 + x[0]
        return [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]

    return f


def _d_rotation(x):
    a = PHI0 + x[0]
    return [[-np.sin(a), -np.cos(a)], [np.cos(a), -np.sin(a)]]


def stratified_solver(phi0=PHI0, nx=3, n=4):
    A = lambda x, y: 1.0 + 0.5 * x[0] + 0.9 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1])
    h = hmm.PoissonStratifiedHMM(mesh.create_unit_square(nx, nx), A, lambda x: 1.0, mesh.create_unit_square(n, n), 0.01, _rotation(phi0),
                                 quadrature_degree=3)
    h._plan = StratOraclePlan(2, n, "poisson")
    return h


def _macro_field(h):
    x = h.function_space.tabulate_dof_coordinates()[:, :2]
    return np.sin(2.0 * x[:, 0]) + x[:, 1] ** 2


def test_stratification_derivatives_shapes_parameters_and_subsets():
    h = stratified_solver()
    nc = h._msh.num_cells
    r = h.stratification_derivatives(parameters=[_d_rotation])
    assert r.dA_dM.shape == (nc, 2, 2, 2, 2) and r.dA.shape == (nc, 1, 2, 2) and r.names == ("_d_rotation",)
    assert np.array_equal(r.cells, np.arange(nc)) and r.grad_M is None and not r.info.any()
    _, M, weights, full = h._plan.seen[0]
    assert full and weights is None and np.array_equal(M, h._stratification(np.arange(nc)))
    dM = np.stack([np.asarray(_d_rotation(c), float) for c in h._msh.cell_midpoints()])
    assert np.abs(r.dA[:, 0] - np.einsum("cab,cabmn->cmn", dM, r.dA_dM)).max() < 1e-14
    # against central differences of the effective tensors of two further solvers
    step = 1e-5
    fd = (stratified_solver(PHI0 + step)._effective_tensors(np.arange(nc))[0] - stratified_solver(PHI0 - step)._effective_tensors(np.arange(nc))[0]) / (2 * step)
    assert np.abs(r.dA[:, 0] - fd).max() < 1e-8 * np.abs(r.A_eff).max()
    plain = h.stratification_derivatives(cells=[4, 1])
    assert plain.dA is None and plain.names is None and np.array_equal(plain.dA_dM, r.dA_dM[[4, 1]]) and np.array_equal(plain.cells, [4, 1])
    with pytest.raises(ValueError, match="at least one"):
        h.stratification_derivatives(cells=[])
    with pytest.raises(ValueError, match="2x2"):
        h.stratification_derivatives(parameters=[lambda x: np.zeros(3)])


def test_unstratified_class_differentiates_at_the_identity():
    A = lambda x, y: 1.0 + 0.9 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1])
    h = hmm.PoissonHMM(mesh.create_unit_square(2, 2), A, lambda x: 1.0, mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
    h._plan = StratOraclePlan(2, 4, "poisson")
    r = h.stratification_derivatives(cells=[0, 3])
    assert h._plan.seen[0][1] is None and r.dA_dM.shape == (2, 2, 2, 2, 2)
    assert np.abs(np.einsum("aa...->...", r.dA_dM[0])).max() < 1e-13 * np.abs(r.A_eff).max()  # homogeneity at M = I


def test_energy_derivatives_equal_the_contraction_of_dA_dM():
    """stratification_energy_derivatives = vol xi_v . dA_dM xi_u, from grad_M alone; and against central differences of v . K_H u."""
    h = stratified_solver()
    nc = h._msh.num_cells
    cells = np.arange(nc)
    u = _macro_field(h)
    v = np.cos(h.function_space.tabulate_dof_coordinates()[:, 0])
    full = h.stratification_derivatives()
    xu, xv = h._macro_strains(cells, u), h._macro_strains(cells, v)
    vol = h._msh.cell_volumes() / h._cell_mesh_area
    h._plan.seen.clear()
    e = h.stratification_energy_derivatives(u, v)
    _, _, weights, asked_full = h._plan.seen[0]
    assert not asked_full and np.array_equal(weights, np.einsum("cm,cn->cmn", xv, xu))  # only grad_M crosses the boundary
    want = vol[:, None, None] * np.einsum("cm,cabmn,cn->cab", xv, full.dA_dM, xu)
    assert e.shape == (nc, 2, 2) and np.abs(e - want).max() < 1e-13 * np.abs(want).max()
    ep = h.stratification_energy_derivatives(u, v, parameters=[_d_rotation])
    dM = np.stack([np.asarray(_d_rotation(c), float) for c in h._msh.cell_midpoints()])
    assert ep.shape == (nc, 1) and np.abs(ep[:, 0] - np.einsum("cab,cab->c", dM, e)).max() < 1e-14 * np.abs(e).max()
    sub = h.stratification_energy_derivatives(u, cells=[5, 2])
    assert np.abs(sub - h.stratification_energy_derivatives(u)[[5, 2]]).max() == 0.0

    def energy(phi0):
        g = stratified_solver(phi0)
        g._assemble_stiffness()
        return v @ (g._A @ u)

    step = 1e-5
    fd = (energy(PHI0 + step) - energy(PHI0 - step)) / (2 * step)
    err = abs(ep.sum() - fd) / abs(fd)
    print("energy derivative against central differences", err)
    assert err < 1e-6
    with pytest.raises(RuntimeError, match="solve"):
        h.stratification_energy_derivatives()
