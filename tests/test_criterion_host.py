"""Failure criteria on the CPU: the grammar of ``Criterion`` (s, e and c beside the names of ``Expression``, which still refuses them),
the ``X`` indices its program reads the state through, ``host_values`` -- the NumPy twin the device is held to -- against formulas
written out in NumPy on dyadic data, and ``BaseHMM.criterion`` on an oracle-backed stand-in plan whose ``criterion`` is its own fields
fed to ``host_values`` (no GPU needed)."""

import numpy as np
import pytest

from hommx_amd import hmm
from hommx_amd.batch import CriterionResult
from hommx_amd.expr import OP_STORE, OP_X, Criterion, Expression
from test_loads_host import LoadOraclePlan, _solver


# -- grammar ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s", "e", "c"])
def test_state_names_are_the_criterions_alone(name):
    assert Criterion(f"{name}[0] + 1").state_indices[name] == 1
    with pytest.raises(ValueError, match="only x and y are indexed"):  # today's text
        Expression(f"{name}[0] + 1")
    with pytest.raises(ValueError, match=f"the index of {name} is a literal integer"):
        Criterion(f"{name}[k]")
    with pytest.raises(ValueError, match=f"the index of {name} is a literal integer"):
        Criterion(f"{name}[21]")


def test_hmm_exports_the_criterion():
    assert hmm.Criterion is Criterion


def test_index_ranges_are_checked_when_the_criterion_meets_a_plan():
    crit = Criterion("s[2] + e[1] + c[1]")
    crit.program(3, 2)
    with pytest.raises(ValueError, match=r"s\[2\] is out of range: the plan has t = 2 \(t = 2, n_comp = 2\)"):
        crit.program(2, 2)
    with pytest.raises(ValueError, match=r"c\[1\] is out of range: the plan has n_comp = 1 \(t = 3, n_comp = 1\)"):
        crit.program(3, 1)
    with pytest.raises(ValueError, match=r"e\[5\] is out of range: the plan has t = 3"):
        Criterion("e[5]").program(3, 21)


def test_the_state_is_read_through_x_on_a_wider_row():
    crit = Criterion("e[1]*s[2] + c[0]*f[1] + x[2]", fields=2)
    for t, n_comp in ((3, 2), (6, 21)):
        ops, consts = crit.program(t, n_comp)
        assert ops.dtype == np.uint8 and [k for op, k in ops if op == OP_X] == [3 + 2 + 1, 3 + 2 + t + 2, 3 + 2 + 2 * t, 3 + 1, 2]
        assert tuple(ops[-1]) == (OP_STORE, 0) and sum(op == OP_STORE for op, _ in ops) == 1  # one component
    assert crit.depth == 3 and crit.n_fields == 2 and crit.n_y == 0


def test_limits_parameters_and_threshold():
    crit = Criterion("p[0]*s[0] + p[1]", p=[2.0, 0.5], parameter_names=("scale", "shift"))
    ops, consts = crit.program(2, 1)
    assert list(consts[:2]) == [2.0, 0.5] and crit.n_params == 2  # the parameters are the first constants
    e = s = np.array([[[0.5, 1.0], [2.0, -1.0]]])
    c, x = np.ones((1, 2)), np.zeros((1, 3))
    assert np.array_equal(crit.host_values(e, s, c, x), [[1.5, 4.5]])
    other = crit.with_parameters([4.0, -1.0])
    assert np.array_equal(other.host_values(e, s, c, x), [[1.0, 7.0]]) and np.array_equal(crit.p, [2.0, 0.5])
    assert np.array_equal(other.program(2, 1)[0], ops)  # nothing is parsed again
    with pytest.raises(ValueError, match="p\\[k\\] needs the values"):
        Criterion("p[0]*s[0]")
    with pytest.raises(ValueError, match="too deep"):
        text = "c[0]"
        for i in range(16):
            text = f"(s[0] + {text})"
        Criterion(text)
    with pytest.raises(ValueError, match="threshold is NaN"):
        Criterion("s[0]", threshold=float("nan"))
    with pytest.raises(ValueError, match="pass fields"):
        Criterion("f[0]*s[0]", fields=1).host_values(e, s, c, x)
    with pytest.raises(ValueError, match="element centroids"):
        Criterion("y[1]*s[0]").host_values(e, s, c, x)


# -- host_values against formulas written out in NumPy, on dyadic data: every operation is exact or the one rounding both sides share --------
def _dyadic(rng, *shape):
    return rng.integers(-16, 17, shape) / 8.0


@pytest.mark.parametrize("kind,dim", [("poisson", 2), ("poisson_matrix", 3), ("elasticity", 2), ("elasticity", 3), ("elasticity_voigt", 3)])
def test_flux_norm(kind, dim):
    rng = np.random.default_rng(1)
    t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
    s = _dyadic(rng, 2, 5, t)
    w = np.array([2.0 if kind.startswith("elasticity") and k >= dim else 1.0 for k in range(t)])
    want = s[..., 0] ** 2
    for k in range(1, t):
        want = want + (w[k] * s[..., k] ** 2 if w[k] != 1.0 else s[..., k] ** 2)
    got = Criterion.flux_norm(kind, dim).host_values(s, s, np.ones((2, 5)), np.zeros((2, 3)))
    assert np.array_equal(got, np.sqrt(want))


def test_von_mises_and_max_principal():
    rng = np.random.default_rng(2)
    e, s, c = _dyadic(rng, 3, 7, 3), _dyadic(rng, 3, 7, 3), np.abs(_dyadic(rng, 3, 7, 2)) + 1
    x = np.zeros((3, 3))
    s0, s1, s2, s33 = s[..., 0], s[..., 1], s[..., 2], c[..., 0] * (e[..., 0] + e[..., 1])
    want = np.sqrt(0.5 * ((s0 - s1) ** 2 + (s1 - s33) ** 2 + (s33 - s0) ** 2) + 3 * (s2 ** 2)) / 1.0
    assert np.array_equal(Criterion.von_mises(2).host_values(e, s, c, x), want)
    plane_stress = np.sqrt(0.5 * ((s0 - s1) ** 2 + (s1 - 0.0) ** 2 + (0.0 - s0) ** 2) + 3 * (s2 ** 2))
    assert np.array_equal(Criterion.von_mises(2, plane="stress").host_values(e, s, c, x), plane_stress)
    strength = np.where(c[..., 1] > 2, 900.0, 60.0)  # a phase-dependent strength through c
    assert np.array_equal(Criterion.von_mises(2, strength="where(c[1] > 2, 900, 60)").host_values(e, s, c, x), want / strength)
    e6, s6 = _dyadic(rng, 3, 7, 6), _dyadic(rng, 3, 7, 6)
    a, b, d = s6[..., 0], s6[..., 1], s6[..., 2]
    want3 = np.sqrt(0.5 * ((a - b) ** 2 + (b - d) ** 2 + (d - a) ** 2) + 3 * (s6[..., 3] ** 2 + s6[..., 4] ** 2 + s6[..., 5] ** 2))
    assert np.array_equal(Criterion.von_mises(3, strength="2").host_values(e6, s6, c, x), want3 / 2.0)
    principal = (0.5 * (s0 + s1) + np.sqrt((0.5 * (s0 - s1)) ** 2 + s2 ** 2)) / 4.0
    assert np.array_equal(Criterion.max_principal(strength="4").host_values(e, s, c, x), principal)
    with pytest.raises(ValueError, match="plane"):
        Criterion.von_mises(2, plane="shear")


def test_where_on_c_with_every_input_class():
    rng = np.random.default_rng(3)
    e, s, c = _dyadic(rng, 2, 4, 2), _dyadic(rng, 2, 4, 2), _dyadic(rng, 2, 4)
    x, y, f = _dyadic(rng, 2, 3), _dyadic(rng, 4, 2), _dyadic(rng, 2, 1)
    crit = Criterion("where(c[0] > 0.5, s[0]*p[0], e[1] - y[1]) + x[0]*f[0]", p=[0.5], fields=1)
    want = np.where(c > 0.5, s[..., 0] * 0.5, e[..., 1] - y[None, :, 1]) + (x[:, 0] * f[:, 0])[:, None]
    assert np.array_equal(crit.host_values(e, s, c, x, y, f), want)
    assert np.array_equal(crit.host_values(e, s, c, x[:, :2], y, f[:, 0]), np.where(c > 0.5, s[..., 0] * 0.5, e[..., 1] - y[None, :, 1]) + (x[:, 0] * f[:, 0])[:, None])


# -- BaseHMM.criterion on a stand-in plan --------------------------------------------------------------------------------------------------
class CriterionOraclePlan(LoadOraclePlan):
    """A stand-in whose criterion() is its own reference fields -- reconstruct() and, with a load, loads() -- fed to host_values."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.crit_calls = []

    def criterion(self, coef, xi, crit, M=None, rows=None, points=None, values=False, fields=False, P=None, per_cell=None, eigenstrain=False):
        self.crit_calls.append((len(coef), None if P is None else np.shape(P), per_cell, np.shape(rows), np.shape(points)))
        r = self.reconstruct(coef, xi, M, fields=True)
        s, q = r.strain, r.flux
        if P is not None:
            lr = self.loads(coef, P, M, per_cell=per_cell, response=True, fields=True)
            s, q = s + lr.strain[:, 0], q + lr.flux[:, 0]
        v = crit.host_values(s, q, coef, rows[:, :3], points, rows[:, 3:])
        vol = 1.0 / v.shape[1]
        return CriterionResult(v.max(axis=1), v.argmax(axis=1), (vol * v).sum(axis=1), (vol * (v >= crit.threshold)).sum(axis=1), r.A_eff,
                               r.info, v if values else None, s if fields else None, q if fields else None)


def _criterion_solver(kind="poisson"):
    h, P, u0, g = _solver(kind)
    h._plan = CriterionOraclePlan(2, 4, kind)
    x = h.function_space.tabulate_dof_coordinates()[:, :2]
    u = np.sin(2.0 * x[:, 0]) + x[:, 1] ** 2 if kind == "poisson" else np.stack([0.1 * x[:, 0] * x[:, 1], -0.2 * x[:, 1] ** 2], axis=1).ravel()
    return h, P, u


FIELDS = ("max", "argmax_element", "mean", "exceed_volume", "values", "strain", "flux", "A_eff", "info")


@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_criterion_is_host_values_of_the_reconstructed_fields(kind):
    h, P, u = _criterion_solver(kind)
    crit = Criterion.flux_norm(kind, 2, threshold=0.75)
    r = h.criterion(crit, u, values=True, fields=True)
    rec = h.reconstruct(u, fields=True)
    assert np.array_equal(r.cells, np.arange(h._msh.num_cells)) and r.values.shape == (h._msh.num_cells, 32)
    assert np.array_equal(r.strain, rec.strain) and np.array_equal(r.flux, rec.flux)
    assert np.allclose(r.max, rec.max_flux, rtol=1e-14) and np.array_equal(r.argmax_element, r.values.argmax(axis=1))
    assert 0 < r.exceed_volume.max() <= 1 and r.exceed_volume.min() < 1
    calls = h._plan.crit_calls
    assert calls == [(h._msh.num_cells, None, None, (h._msh.num_cells, 3), (32, 2))]  # the midpoints and the element centroids
    lean = h.criterion(crit, u)
    assert lean.values is None and lean.strain is None and np.array_equal(lean.mean, r.mean)


def test_chunk_boundaries_and_fields():
    h, P, u = _criterion_solver()
    n = h._msh.num_cells
    strength = 1.0 + np.arange(n) / n
    crit = Criterion("sqrt(s[0]**2 + s[1]**2) / f[0] + 0.125*y[0] + x[1]", fields=("strength",), threshold=1.5)
    full = h.criterion(crit, u, field_values=strength, values=True, fields=True)
    h._plan.crit_calls.clear()
    parts = h.criterion(crit, u, field_values=strength, values=True, fields=True, chunk_cells=25)
    assert [c[0] for c in h._plan.crit_calls] == [25, 25, n - 50] and all(c[3] == (c[0], 4) for c in h._plan.crit_calls)
    for name in FIELDS:
        assert np.array_equal(getattr(full, name), getattr(parts, name)), name
    some = np.array([5, 1, 40])
    sub = h.criterion(crit, u, cells=some, field_values=lambda x: 1.0 + (np.arange(n) / n), values=True)
    assert np.array_equal(sub.values, full.values[some]) and np.array_equal(sub.cells, some)
    other = h.criterion(crit, u, field_values=2 * strength, values=True)  # the field is read: twice the strength
    assert not np.array_equal(other.values, full.values)


@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_load_none_false_true(kind):
    h, P, u = _criterion_solver(kind)
    crit = Criterion.flux_norm(kind, 2)
    with pytest.raises(RuntimeError, match="needs a polarisation"):
        h.criterion(crit, u, load=True)
    bare = h.criterion(crit, u, values=True, fields=True)
    assert np.array_equal(h.criterion(crit, u, load=False, values=True).values, bare.values)
    h.set_polarisation(P)
    rec, lr = h.reconstruct(u, fields=True, chunk_cells=7), h.load_response(fields=True, chunk_cells=7)  # the chunks of the call below
    for load in (None, True):
        r = h.criterion(crit, u, load=load, values=True, fields=True, chunk_cells=7)
        assert np.array_equal(r.flux, rec.flux + lr.flux[:, 0]) and np.array_equal(r.strain, rec.strain + lr.strain[:, 0])
        assert np.array_equal(r.values, crit.host_values(r.strain, r.flux, h._element_means(r.cells)[0], h._msh.cell_midpoints()))
        assert not np.array_equal(r.values, bare.values)
    assert h._plan.crit_calls[-1][1:3] == ((h._msh.num_cells % 7 or 7, 1, 32, h._plan.t), True)  # a sampled load, per cell
    mech = h.criterion(crit, u, load=False, values=True)
    assert np.array_equal(mech.values, bare.values)


def test_the_two_runtime_errors_and_the_macro_solution():
    h, P, u = _criterion_solver()
    with pytest.raises(RuntimeError, match="field_values"):
        h.criterion(Criterion("s[0]*f[0]", fields=1), u)
    with pytest.raises(RuntimeError, match="needs a polarisation"):
        h.criterion(Criterion("s[0]"), u, load=True)
    with pytest.raises(RuntimeError, match="call solve\\(\\) first or pass u"):
        h.criterion(Criterion("s[0]"))
    with pytest.raises(ValueError, match="shape"):
        h.criterion(Criterion("s[0]*f[0]", fields=1), u, field_values=np.ones(3))
