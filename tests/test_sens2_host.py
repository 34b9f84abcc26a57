"""Second derivatives of A_H along coefficient directions on the CPU: the NumPy / SciPy reference (tests/sens2_ref.py)
checked against itself -- the energy form against the direct form, Euler, concavity, bilinearity -- and against central second differences
of the CPU oracle's A_H before anything leans on it; the argument checks of hommx_second_sensitivity_source[_device] (they run before any
device is touched); the solver classes on a stub plan that answers from the reference (no GPU needed)."""

import ctypes
import os

import numpy as np
import pytest

import sens2_ref as S2
from hommx_amd import _lib, hmm, mesh
from hommx_amd.batch import CoefStream, SecondSensitivities
from test_reconstruct_host import ReconOraclePlan
from test_reconstruct_source_host import _fake_plan

KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")
# all four kinds in 2D, Poisson and elasticity in 3D, each with and without M
SHAPES = [(kind, 2, 5) for kind in KINDS] + [("poisson", 3, 3), ("elasticity", 3, 3)]
CASES = [(kind, dim, n, strat) for kind, dim, n in SHAPES for strat in (True, False)]


def _case(kind, dim, n, strat, n_dirs=3):
    """A contrast-1e2 cell and ``n_dirs`` random directions of the size of its coefficient (coef times uniform(-1, 1) per entry)."""
    rng = np.random.default_rng(CASES.index((kind, dim, n, strat)))
    n_el = (2 if dim == 2 else 6) * n**dim
    coef = S2.random_coef(kind, dim, n_el, rng)
    M = S2.random_M(dim, rng) if strat else None
    dirs = np.stack([coef * rng.uniform(-1.0, 1.0, coef.shape) for _ in range(n_dirs)])
    return coef, M, dirs


# -- 1. the reference against itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,n,strat", CASES)
def test_reference_checks_itself(kind, dim, n, strat):
    coef, M, dirs = _case(kind, dim, n, strat)
    cell = S2.structured(kind, dim, n, coef, M)
    d2A = S2.second_derivatives(cell, dirs)
    scale = np.abs(d2A).max()
    assert d2A.shape == (3, 3, cell.t, cell.t) and scale > 0
    # the energy form and the direct form are the same sums in exact arithmetic and share none (observed: <= 2e-15)
    err = np.abs(d2A - S2.second_derivatives(cell, dirs, "direct")).max() / scale
    print(kind, dim, n, strat, "energy form against direct form", err)
    assert err < 1e-12
    assert np.array_equal(d2A, np.transpose(d2A, (1, 0, 2, 3))) and np.abs(d2A - np.transpose(d2A, (0, 1, 3, 2))).max() < 1e-13 * scale
    # Euler: A_H is 1-homogeneous, the corrector derivative along the coefficient itself is zero
    eu = S2.second_derivatives(cell, np.stack([coef, dirs[0]]))
    assert np.abs(eu[0]).max() < 1e-12 * np.abs(eu).max() and np.abs(eu[:, 0]).max() < 1e-12 * np.abs(eu).max()
    assert np.abs(S2.load_strains(cell, coef[None])).max() < 1e-12
    # concavity: every diagonal block is negative semidefinite
    for a in range(3):
        assert np.linalg.eigvalsh(d2A[a, a]).max() <= 1e-12 * scale
    # bilinearity
    third = S2.second_derivatives(cell, np.stack([dirs[0], dirs[1], 2.0 * dirs[0] - dirs[1]]))
    want = 4.0 * third[0, 0] - 4.0 * third[0, 1] + third[1, 1]
    assert np.abs(third[2, 2] - want).max() < 1e-12 * np.abs(third).max()
    # the first derivatives of the same cell: the direction coef gives A_H
    assert np.abs(S2.first_derivatives(cell, coef[None])[0] - cell.A).max() < 1e-12 * np.abs(cell.A).max()


# -- 2. central second differences ---------------------------------------------------------------------------------------------------------
H = 2e-4
FD_BOUND = 5e-5


@pytest.mark.parametrize("kind,dim,n,strat", [("poisson", 2, 5, False), ("poisson", 2, 6, True), ("elasticity", 2, 4, True), ("poisson", 3, 3, True),
                                              ("elasticity", 3, 3, False)])
def test_reference_matches_central_second_differences(kind, dim, n, strat):
    """The exact form against central second differences of the CPU oracle's A_H (Schur form: another assembly and another solve) at
    h = 2e-4, relative to max |d2A|.  The bound 5e-5 is about 3.6 x the largest error of such differences measured when the feature was
    specified (1.4e-5, a truncation error, which scales with h^2): the differences, not the exact form, set it.  With the directions of
    this file (of the size of the coefficient) the observed error is 5e-8 .. 6e-7, and at this step it is the differences' rounding
    (eps |A_H| / h^2: it grows when h falls) -- either way far above the 1e-15 at which the two exact forms agree."""
    rng = np.random.default_rng(100 + dim * n)
    n_el = (2 if dim == 2 else 6) * n**dim
    coef = S2.random_coef(kind, dim, n_el, rng)
    M = S2.random_M(dim, rng) if strat else None
    dirs = np.stack([coef * rng.uniform(-1.0, 1.0, coef.shape) for _ in range(3)])
    d2A = S2.second_derivatives(S2.structured(kind, dim, n, coef, M), dirs)
    fd = S2.central_second_differences(kind, dim, n, coef, M, dirs, H)
    err = np.abs(fd - d2A).max() / np.abs(d2A).max()
    print(kind, dim, n, strat, "exact form against central second differences", err)
    assert err < FD_BOUND


# -- 3. C ABI argument checks ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _fake_mesh_plan(kind, flags):
    """Plan-shaped memory whose descriptor is that of a mesh plan (n_micro == 0) of the frontal (flags 0) or the tree route."""
    fake = ctypes.create_string_buffer(4096)
    ctypes.memmove(fake, ctypes.byref(_lib.PlanDesc(2, 0, kind, 0, flags)), ctypes.sizeof(_lib.PlanDesc))
    return fake


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_second_sensitivity_source_device if device_entry else lib.hommx_second_sensitivity_source
    tail = (None,) if device_entry else ()

    def call(plan, src, args, n_cells=1):
        rc = fn(plan, n_cells, src, None, None if args is None else ctypes.byref(args), *tail)
        return rc, lib.hommx_last_error().decode()

    def args(**kw):
        return _lib.Sens2Args(**dict(dict(n_dirs=2, per_cell=0, dirs=p, d2A=p), **kw))

    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    for kind in (_lib.KIND_POISSON_SCALAR, _lib.KIND_ELASTICITY_ISO):
        fake = _fake_plan(kind)
        plan = ctypes.addressof(fake)
        assert lib.hommx_plan_kind(plan) == kind
        rc, msg = call(None, sampled, args())
        assert rc == -1 and "null plan" in msg
        assert call(None, sampled, args(), n_cells=0)[0] == -1  # a null plan, even when empty
        rc, msg = call(plan, sampled, args(), n_cells=-1)
        assert rc == -1 and "negative n_cells" in msg
        assert call(plan, None, None, n_cells=0)[0] == 0  # an empty batch reads nothing
        rc, msg = call(plan, None, args())
        assert rc == -1 and "null source" in msg
        rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=7, coef=p)), args())
        assert rc == -1 and "unknown coefficient form 7" in msg
        rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=_lib.COEF_TWO_PHASE, mask=p)), args())
        assert rc == -1 and "null mask / values" in msg
        rc, msg = call(plan, sampled, None)
        assert rc == -1 and msg == "null arguments"
        for nd in (0, -2, _lib.SENS_MAX_DIRS + 1):
            rc, msg = call(plan, sampled, args(n_dirs=nd))
            assert rc == -1 and msg == f"n_dirs must be 1 .. {_lib.SENS_MAX_DIRS}, got {nd}"
        for kw in ({"dirs": None}, {"d2A": None}):
            rc, msg = call(plan, sampled, args(**kw))
            assert rc == -1 and msg == "null dirs / d2A"
        # a plan of the frontal mesh route is refused on its descriptor, before anything else of it is read
        front = _fake_mesh_plan(kind, 0)
        rc, msg = call(ctypes.addressof(front), sampled, args())
        assert rc == -1 and "frontal mesh route" in msg and "tree route" in msg and 'route="tree"' in msg and "HOMMX_MESH_FLAG_TREE" in msg
        assert call(ctypes.addressof(front), sampled, args(n_dirs=0))[1].startswith("n_dirs must be")  # after the argument struct's own checks
    if device_entry:
        rc, msg = call(plan, sampled, args(), n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg


# -- 4. solver classes on a stub plan that answers from the reference ------------------------------------------------------------------------
class Sens2OraclePlan(ReconOraclePlan):
    """solve() of the oracle-backed stand-in, and second_sensitivities() from tests/sens2_ref.py; records what it was given."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.seen = []

    def second_sensitivities(self, coef, M=None, directions=None, per_cell=False, first=False):
        self.seen.append((coef, directions, per_cell, first))
        if isinstance(coef, CoefStream):
            assert coef.method == "solve_two_phase"
            coef = coef.per_cell[:, coef.shared[0].astype(int)]
        cells = [S2.structured(self.kind, self.dim, self.n, coef[k], None if M is None else M[k]) for k in range(len(coef))]
        dirs = lambda k: directions[k] if per_cell else directions
        d2A = np.stack([S2.second_derivatives(c, dirs(k)) for k, c in enumerate(cells)])
        dA = np.stack([S2.first_derivatives(c, dirs(k)) for k, c in enumerate(cells)]) if first else None
        return SecondSensitivities(d2A, dA, np.stack([c.A for c in cells]), np.zeros(len(coef), np.int32))


INSIDE = lambda x: 5.0 + 2.0 * x[0]


def two_phase_solver(nx=3, n=4):
    A = hmm.TwoPhase(lambda y: (y[0] > 0.25) & (y[0] < 0.75) & (y[1] < 0.5), INSIDE, lambda x: 1.0 + 0.0 * x[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: 1.0, mesh.create_unit_square(n, n), 0.01)
    h._plan = Sens2OraclePlan(2, n, "poisson")
    return h


def test_two_phase_names_shapes_and_euler():
    h = two_phase_solver()
    r = h.tensor_second_derivatives()
    nc = h._msh.num_cells
    assert r.names == ("outside", "inside") and r.d2A.shape == (nc, 2, 2, 2, 2) and r.dA.shape == (nc, 2, 2, 2)
    assert r.A_eff.shape == (nc, 2, 2) and not r.info.any() and np.array_equal(r.cells, np.arange(nc))
    coef, dirs, per_cell, first = h._plan.seen[0]
    assert isinstance(coef, np.ndarray) and dirs.shape == (2, 32) and not per_cell and first  # shared indicator directions
    assert np.array_equal(dirs[0] + dirs[1], np.ones(32)) and np.array_equal(dirs[1] == 1.0, h._phase_mask())
    # Euler on the two values: the gradient is 0-homogeneous, so outside d2A[:, a, 0] + inside d2A[:, a, 1] = 0
    vin = INSIDE(h._msh.cell_midpoints().T)
    back = 1.0 * r.d2A[:, :, 0] + vin[:, None, None, None] * r.d2A[:, :, 1]
    assert np.abs(back).max() < 1e-12 * np.abs(r.d2A).max()
    assert np.abs(1.0 * r.dA[:, 0] + vin[:, None, None] * r.dA[:, 1] - r.A_eff).max() < 1e-12 * np.abs(r.A_eff).max()
    sub = h.tensor_second_derivatives(cells=[4, 1], chunk_cells=1)
    assert len(h._plan.seen) == 3 and np.array_equal(sub.d2A, r.d2A[[4, 1]]) and np.array_equal(sub.cells, [4, 1])


def test_two_phase_elasticity_names():
    tp = hmm.TwoPhase(lambda y: y[0] < 0.5, lambda x: hmm.Lame(2.0 + x[0], 3.0 + 0 * x[0]), lambda x: hmm.Lame(1.0 + 0 * x[0], 0.5 + 0 * x[0]))
    h = hmm.LinearElasticityHMM(mesh.create_unit_square(2, 2), tp, lambda x: np.zeros(2), mesh.create_unit_square(3, 3), 0.01)
    h._plan = Sens2OraclePlan(2, 3, "elasticity")
    r = h.tensor_second_derivatives(cells=[0, 5])
    assert r.names == ("outside.lambda", "outside.mu", "inside.lambda", "inside.mu") and r.d2A.shape == (2, 4, 4, 3, 3)
    values = tp.phase_values(h._msh.cell_midpoints()[[0, 5]])  # [2 cells, 2 phases, (lambda, mu)]
    assert np.abs(np.einsum("cb,cabmn->camn", values.reshape(2, 4), r.d2A)).max() < 1e-12 * np.abs(r.d2A).max()


def test_directions_from_callables_go_per_cell():
    h = two_phase_solver()
    d0 = lambda x, y: (1.0 + x[0]) * np.sin(2 * np.pi * y[0]) ** 2
    r = h.tensor_second_derivatives(cells=[2, 7, 11], directions=[d0, h._coeff])
    assert r.d2A.shape == (3, 2, 2, 2, 2) and r.names[0] == "<lambda>" and len(r.names) == 2
    coef, dirs, per_cell, _ = h._plan.seen[0]
    assert per_cell and dirs.shape == (3, 2, 32) and np.array_equal(dirs[:, 1], coef)
    scale = np.abs(r.d2A).max()
    assert np.abs(r.d2A[:, 1]).max() < 1e-12 * scale and np.abs(r.d2A[:, :, 1]).max() < 1e-12 * scale and scale > 0


def test_value_errors():
    rec = hmm.PoissonHMM(mesh.create_unit_square(2, 2), hmm.Separable("reciprocal", lambda x: 2.0, lambda x: 1.0, lambda y: np.cos(2 * np.pi * y[0])),
                         lambda x: 1.0, mesh.create_unit_square(4, 4), 0.01)
    rec._plan = Sens2OraclePlan(2, 4, "poisson")
    with pytest.raises(ValueError, match="directions="):
        rec.tensor_second_derivatives()
    with pytest.raises(ValueError, match="at least one"):
        two_phase_solver().tensor_second_derivatives(cells=[])
    with pytest.raises(RuntimeError, match="solve"):
        two_phase_solver().energy_second_derivatives()


def test_energy_second_derivatives_equal_the_host_contraction():
    h = two_phase_solver()
    x = h.function_space.tabulate_dof_coordinates()[:, :2]
    u, v = np.sin(2.0 * x[:, 0]) + x[:, 1] ** 2, np.cos(x[:, 0])
    r = h.tensor_second_derivatives()
    cells = np.arange(h._msh.num_cells)
    vol = h._msh.cell_volumes() / h._cell_mesh_area
    xu, xv = h._macro_strains(cells, u), h._macro_strains(cells, v)
    e = h.energy_second_derivatives(u)
    assert e.shape == (len(cells), 2, 2)
    assert np.array_equal(e, vol[:, None, None] * np.einsum("cm,cabmn,cn->cab", xu, r.d2A, xu))
    assert np.all(e[:, [0, 1], [0, 1]] <= 1e-12 * np.abs(e).max())  # the frozen-u energy is concave in every parameter
    ev = h.energy_second_derivatives(u, v, cells=[3, 0])
    want = (vol[:, None, None] * np.einsum("cm,cabmn,cn->cab", xv, r.d2A, xu))[[3, 0]]
    assert np.abs(ev - want).max() <= 1e-14 * np.abs(want).max()
