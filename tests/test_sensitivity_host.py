"""Derivatives of A_H along coefficient directions on the CPU: the NumPy reference (tests/sens_ref.py) against central differences of the
oracle's A_H and its exact identities, the argument checks of hommx_sensitivity_source[_device] (they run before any device is touched),
and BaseHMM.tensor_derivatives / energy_derivatives on stub plans that answer from the reference (no GPU needed)."""

import ctypes
import functools
import os

import numpy as np
import pytest

import recon_ref as R
import sens_ref as S
from hommx_amd import _lib, hmm, mesh
from hommx_amd.batch import CoefStream, Sensitivities
from test_reconstruct_host import ReconOraclePlan

# the six cases the formula was checked on: kind, dim, n
CASES = [("poisson", 2, 5), ("poisson_matrix", 2, 4), ("elasticity", 2, 4), ("elasticity_voigt", 2, 3), ("elasticity", 3, 3), ("poisson", 3, 3)]


@functools.lru_cache(maxsize=None)
def _case(k):
    """Random coefficient of contrast 1e2 with a random M, its reference cell, a direction of 10 % of the coefficient and weights."""
    kind, dim, n = CASES[k]
    rng = np.random.default_rng(100 + k)
    n_el = (2 if dim == 2 else 6) * n**dim
    coef = R.random_coef(kind, dim, n_el, rng)
    M = R.random_M(dim, rng)
    cell = S.structured(kind, dim, n, coef, M)
    delta = 0.1 * coef * rng.uniform(-1.0, 1.0, coef.shape)
    w = rng.standard_normal((cell.t, cell.t))
    return coef, M, cell, delta, w


@pytest.mark.parametrize("k", range(len(CASES)))
def test_reference_against_central_difference_of_the_oracle(k):
    """h = 1e-5 along 10 % of the coefficient: the truncation term h^2 A''' / 6 grows with the contrast, the figures on these cases are
    5e-10 .. 2e-8."""
    kind, dim, n = CASES[k]
    coef, M, cell, delta, _ = _case(k)
    h = 1e-5
    fd = (S.oracle_tensor(kind, dim, n, coef + h * delta, M) - S.oracle_tensor(kind, dim, n, coef - h * delta, M)) / (2 * h)
    dA = cell.dA(delta)
    err = np.abs(fd - dA).max() / np.abs(dA).max()
    print(CASES[k], "central difference", err)
    assert err < 1e-6


@pytest.mark.parametrize("k", range(len(CASES)))
def test_reference_identities(k):
    """Euler (A_H is 1-homogeneous in the coefficient): dA[coef] = A_H; and sum grad . delta = w : dA[delta]."""
    coef, M, cell, delta, w = _case(k)
    euler = np.abs(cell.dA(coef) - cell.A).max() / np.abs(cell.A).max()
    n_comp = coef.reshape(len(cell.vol), -1).shape[1]
    terms = cell.grad(w, n_comp) * delta.reshape(len(cell.vol), -1)
    pairing = abs(terms.sum() - (w * cell.dA(delta)).sum()) / np.abs(terms).sum()
    print(CASES[k], "euler", euler, "pairing", pairing)
    assert euler < 1e-12 and pairing < 1e-12
    dA = cell.dA(delta)
    assert np.abs(dA - dA.T).max() < 1e-12 * np.abs(dA).max()


# -- C ABI argument checks ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    """Every fault is reported on plan-shaped memory whose descriptor alone is read: no device is touched."""
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_sensitivity_source_device if device_entry else lib.hommx_sensitivity_source
    tail = (None,) if device_entry else ()

    def call(plan, src, args, n_cells=1):
        rc = fn(plan, n_cells, src, None, None if args is None else ctypes.byref(args), *tail)
        return rc, lib.hommx_last_error().decode()

    fake = ctypes.create_string_buffer(4096)
    ctypes.memmove(fake, ctypes.byref(_lib.PlanDesc(2, 8, _lib.KIND_POISSON_SCALAR, 0, 0)), ctypes.sizeof(_lib.PlanDesc))
    plan = ctypes.addressof(fake)
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    good = _lib.SensArgs(n_dirs=2, dirs=p, dA=p)
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
    for nd in (-1, _lib.SENS_MAX_DIRS + 1):
        rc, msg = call(plan, sampled, _lib.SensArgs(n_dirs=nd, dirs=p, dA=p))
        assert rc == -1 and "n_dirs must be 0 .. 8" in msg, nd
    for args in (_lib.SensArgs(n_dirs=1, dirs=p), _lib.SensArgs(n_dirs=1, dA=p), _lib.SensArgs(n_dirs=3, weights=p, grad=p)):
        rc, msg = call(plan, sampled, args)
        assert rc == -1 and "needs both dirs and dA" in msg
    for args in (_lib.SensArgs(n_dirs=1, dirs=p, dA=p, weights=p), _lib.SensArgs(n_dirs=0, grad=p)):
        rc, msg = call(plan, sampled, args)
        assert rc == -1 and "weights and grad: both or neither" in msg
    rc, msg = call(plan, sampled, _lib.SensArgs(n_dirs=0, A_eff=p))
    assert rc == -1 and "nothing requested" in msg
    assert call(plan, sampled, _lib.SensArgs(), n_cells=0)[0] == 0  # an empty batch asks for nothing


# -- solver classes on stub plans that answer from the reference ---------------------------------------------------------------------------
class SensOraclePlan(ReconOraclePlan):
    """solve() of the oracle-backed stand-in, and sensitivities() from tests/sens_ref.py; records what it was given."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.seen = []

    def sensitivities(self, coef, M=None, directions=None, per_cell=False, weights=None):
        self.seen.append((coef, directions, per_cell))
        if isinstance(coef, CoefStream):
            assert coef.method == "solve_two_phase"
            coef = coef.per_cell[:, coef.shared[0].astype(int)]
        cells = [S.structured(self.kind, self.dim, self.n, coef[k], None if M is None else M[k]) for k in range(len(coef))]
        dA = np.stack([np.stack([c.dA(d) for d in (directions[k] if per_cell else directions)]) for k, c in enumerate(cells)])
        return Sensitivities(dA, None, np.stack([c.A for c in cells]), np.zeros(len(coef), np.int32))


class SensSamplerPlan(SensOraclePlan):
    """... with the sampler method of the two-phase form, so the solver classes hand it that form as the CoefStream."""

    def solve_two_phase(self, mask, values, M=None, return_info=False):
        return self.solve(values[:, np.asarray(mask).astype(int)], M, return_info)


INSIDE = lambda x: 5.0 + 2.0 * x[0]


def two_phase_solver(plan_cls=SensOraclePlan, scale=1.0, nx=3, n=4):
    A = hmm.TwoPhase(lambda y: (y[0] > 0.25) & (y[0] < 0.75) & (y[1] < 0.5), lambda x: scale * INSIDE(x), lambda x: 1.0 + 0.0 * x[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: 1.0, mesh.create_unit_square(n, n), 0.01)
    h._plan = plan_cls(2, n, "poisson")
    return h


def _macro_field(h):
    x = h.function_space.tabulate_dof_coordinates()[:, :2]
    return np.sin(2.0 * x[:, 0]) + x[:, 1] ** 2


def test_two_phase_names_shapes_and_euler():
    h = two_phase_solver()
    r = h.tensor_derivatives()
    nc = h._msh.num_cells
    assert r.names == ("outside", "inside") and r.dA.shape == (nc, 2, 2, 2) and np.array_equal(r.cells, np.arange(nc))
    coef, dirs, per_cell = h._plan.seen[0]
    assert isinstance(coef, np.ndarray) and dirs.shape == (2, 32) and not per_cell  # shared indicator directions, element means
    assert np.array_equal(dirs[0] + dirs[1], np.ones(32)) and np.array_equal(dirs[1] == 1.0, h._phase_mask())
    # A_H = outside dA/d outside + inside dA/d inside (Euler on the two values)
    vin = INSIDE(h._msh.cell_midpoints().T)
    back = 1.0 * r.dA[:, 0] + vin[:, None, None] * r.dA[:, 1]
    assert np.abs(back - r.A_eff).max() < 1e-12 * np.abs(r.A_eff).max()
    sub = h.tensor_derivatives(cells=[4, 1])
    assert np.array_equal(sub.dA, r.dA[[4, 1]]) and np.array_equal(sub.cells, [4, 1])


def test_device_sampled_coefficient_is_not_evaluated_on_the_host(monkeypatch):
    h = two_phase_solver(SensSamplerPlan)

    def no_means(self, cells, coeff=None):
        raise AssertionError("a device-sampled coefficient must not be sampled on the host")

    monkeypatch.setattr(hmm.BaseHMM, "_element_means", no_means)
    r = h.tensor_derivatives()
    coef, _, _ = h._plan.seen[0]
    assert isinstance(coef, CoefStream) and coef.method == "solve_two_phase" and coef.per_cell.shape == (h._msh.num_cells, 2)
    monkeypatch.undo()
    assert np.array_equal(r.dA, two_phase_solver().tensor_derivatives().dA)


def test_two_phase_elasticity_names():
    tp = hmm.TwoPhase(lambda y: y[0] < 0.5, lambda x: hmm.Lame(2.0 + x[0], 3.0 + 0 * x[0]), lambda x: hmm.Lame(1.0 + 0 * x[0], 0.5 + 0 * x[0]))
    h = hmm.LinearElasticityHMM(mesh.create_unit_square(2, 2), tp, lambda x: np.zeros(2), mesh.create_unit_square(3, 3), 0.01)
    h._plan = SensOraclePlan(2, 3, "elasticity")
    r = h.tensor_derivatives(cells=[0, 5])
    assert r.names == ("outside.lambda", "outside.mu", "inside.lambda", "inside.mu") and r.dA.shape == (2, 4, 3, 3)
    values = tp.phase_values(h._msh.cell_midpoints()[[0, 5]])  # [2 cells, 2 phases, (lambda, mu)]
    back = np.einsum("cd,cdmn->cmn", values.reshape(2, 4), r.dA)
    assert np.abs(back - r.A_eff).max() < 1e-12 * np.abs(r.A_eff).max()


def test_affine_names_shapes_and_euler():
    a, b, g = (lambda x: 2.0 + x[0]), (lambda x: 0.5 + 0.25 * x[1]), (lambda y: np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1]))
    h = hmm.PoissonHMM(mesh.create_unit_square(2, 2), hmm.Separable("affine", a, b, g), lambda x: 1.0, mesh.create_unit_square(4, 4), 0.01)
    h._plan = SensOraclePlan(2, 4, "poisson")
    r = h.tensor_derivatives()
    assert r.names == ("a", "b") and r.dA.shape == (8, 2, 2, 2)
    _, dirs, per_cell = h._plan.seen[0]
    yq, w = h._quadrature_points()
    assert not per_cell and np.array_equal(dirs[0], np.ones(32)) and np.array_equal(dirs[1], h._coeff.table(yq, w))
    c = h._msh.cell_midpoints().T
    back = a(c)[:, None, None] * r.dA[:, 0] + b(c)[:, None, None] * r.dA[:, 1]
    assert np.abs(back - r.A_eff).max() < 1e-12 * np.abs(r.A_eff).max()


def test_directions_from_callables_go_per_cell():
    h = two_phase_solver()
    d0 = lambda x, y: (1.0 + x[0]) * np.sin(2 * np.pi * y[0]) ** 2
    r = h.tensor_derivatives(cells=[2, 7, 11], directions=[d0, h._coeff])
    assert r.dA.shape == (3, 2, 2, 2) and r.names[0] == "<lambda>" and len(r.names) == 2
    coef, dirs, per_cell = h._plan.seen[0]
    assert per_cell and dirs.shape == (3, 2, 32)
    # sampled exactly as the coefficient is: the coefficient itself as a direction is its element means, and gives A_H (Euler)
    assert np.array_equal(dirs[:, 1], coef)
    assert np.abs(r.dA[:, 1] - r.A_eff).max() < 1e-12 * np.abs(r.A_eff).max()
    yq, w = h._quadrature_points()
    want = np.stack([d0(c, yq.reshape(-1, 2).T).reshape(32, -1) @ w for c in h._msh.cell_midpoints()[[2, 7, 11]]])
    assert np.abs(dirs[:, 0] - want).max() < 1e-14


def test_value_errors():
    rec = hmm.PoissonHMM(mesh.create_unit_square(2, 2), hmm.Separable("reciprocal", lambda x: 2.0, lambda x: 1.0, lambda y: np.cos(2 * np.pi * y[0])),
                         lambda x: 1.0, mesh.create_unit_square(4, 4), 0.01)
    plain = hmm.PoissonHMM(mesh.create_unit_square(2, 2), lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]), lambda x: 1.0,
                           mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
    for h in (rec, plain):
        h._plan = SensOraclePlan(2, 4, "poisson")
        with pytest.raises(ValueError, match="directions="):
            h.tensor_derivatives()
    with pytest.raises(ValueError, match="coefficient's shape"):  # a matrix-valued direction of a scalar coefficient
        plain.tensor_derivatives(directions=[lambda x, y: np.broadcast_to(np.eye(2), (y.shape[1], 2, 2))])
    with pytest.raises(ValueError, match="at least one"):
        plain.tensor_derivatives(cells=[])
    with pytest.raises(RuntimeError, match="solve"):
        two_phase_solver().energy_derivatives()


def test_energy_derivatives_against_central_difference_of_the_macro_energy():
    """E(theta) = u . K_H(theta) u at frozen u, with the inside value scaled by theta: dE/d theta at 1 = sum_T inside(x_T) dE_T/d inside."""
    h = two_phase_solver()
    u = _macro_field(h)
    e = h.energy_derivatives(u)
    assert e.shape == (h._msh.num_cells, 2)
    vin = INSIDE(h._msh.cell_midpoints().T)

    def energy(scale, v=u):
        g = two_phase_solver(scale=scale)
        g._assemble_stiffness()
        return v @ (g._A @ u)

    step = 1e-5
    fd = (energy(1 + step) - energy(1 - step)) / (2 * step)
    err = abs((vin * e[:, 1]).sum() - fd) / abs(fd)
    print("energy derivative against central difference", err)
    assert err < 1e-6
    # Euler on both values: the energy itself
    assert abs((e[:, 0] + vin * e[:, 1]).sum() - energy(1.0)) < 1e-12 * abs(energy(1.0))
    # the adjoint product with another field
    v = np.cos(h.function_space.tabulate_dof_coordinates()[:, 0])
    ev = h.energy_derivatives(u, v)
    fd = (energy(1 + step, v) - energy(1 - step, v)) / (2 * step)
    assert abs((vin * ev[:, 1]).sum() - fd) < 1e-6 * abs(fd)
