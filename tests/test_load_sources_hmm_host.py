"""Polarisation and eigenstrain loads of the solver classes on the CPU, on oracle-backed stand-in plans as
tests/test_loads_host.py uses them: a vector ``Expression`` as the polarisation, ``set_eigenstrain`` in every form it takes,
``set_polarisation_fields``, what crosses to a plan that takes load sources and to one that does not, and the host statement of
``material()``.  No GPU needed."""

import numpy as np
import pytest

import load_sources_cases as S
import loads_ref as L
from hommx_amd import hmm
from hommx_amd.batch import CoefStream
from hommx_amd.expr import Expression
from test_loads_host import LoadOraclePlan

N_MICRO = {"poisson": 8, "elasticity": 6}  # the sizes of the device tests: what is measured here is what they lean on


class SourcePlan(LoadOraclePlan):
    """A stand-in that says it takes load sources: it records what ``loads`` was given, and answers a program ``CoefStream`` through the
    host interpreter of the expression the test names (``expression``) and an eigenstrain through ``hmm.eigenstress``."""

    load_sources = True
    expression = None

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.given = []

    def loads(self, coef, P, M=None, per_cell=None, **kw):
        self.given.append((P, per_cell, dict(kw)))
        eigenstrain = kw.pop("eigenstrain", False)
        if isinstance(P, CoefStream):
            points, weights, prog = P.shared
            assert np.array_equal(self.expression.program()[0], prog.ops) and np.array_equal(self.expression.program()[1], prog.consts)
            assert (prog.n_comp, prog.n_params, prog.n_fields) == (self.t, self.expression.n_params, self.expression.n_fields)
            P, per_cell = self.expression.host_stream(P.per_cell, points, weights)[:, None], True
        if eigenstrain:
            P = hmm.eigenstress(coef[:, None], self.kind, self.dim, P if per_cell else P[None])
            per_cell = True
        return super().loads(coef, P, M, per_cell=per_cell, **kw)


def _problem(kind, plan=LoadOraclePlan):
    h, E, P, g, Ec = S.PROBLEMS[kind]()
    h._plan = plan(2, N_MICRO[kind], kind)
    return h, E, P, g, Ec


def _run(h, g):
    return S.solve(h, g), h.effective_polarisation.copy()


def _close(a, b, tol, what):
    for got, want, name in zip(a, b, ("u", "P_eff")):
        err = S.difference(got, want)
        print(f"{what}: {name} differs by {err:.3e}")
        assert err <= tol, (what, name, err)


# -- the host statement of material() ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["poisson", "poisson_matrix", "elasticity", "elasticity_voigt"])
@pytest.mark.parametrize("dim", [2, 3])
def test_material_matrix_is_the_references(kind, dim):
    rng = np.random.default_rng(dim + 10 * len(kind))
    n_el, t = 7, L.tensor_size(kind, dim)
    coef = L.random_coef(kind, dim, n_el, rng)
    V = L.voigt_material(kind, coef, dim, n_el)
    C = hmm.material_matrix(coef, kind, dim)
    assert C.shape == (n_el, t, t) and np.abs(C - V).max() <= 1e-14 * np.abs(V).max()
    E = rng.standard_normal((3, n_el, t))
    assert np.allclose(hmm.eigenstress(coef, kind, dim, E), -np.einsum("emn,len->lem", V, E), rtol=1e-13, atol=0)
    assert hmm.eigenstress(coef[None, None], kind, dim, E[None]).shape == (1, 3, n_el, t)  # the leading axes broadcast


# -- a stand-in without the capability -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_expression_polarisation_equals_the_callable_on_a_stand_in(kind):
    h, E, _, g, Ec = _problem(kind)
    h.set_polarisation(Ec)  # the eigenstrain's texts serve as a polarisation here: any vector field does
    want = _run(h, g)
    h.set_polarisation(E)
    with pytest.raises(RuntimeError, match="set_polarisation_fields"):
        h.solve()
    with pytest.raises(RuntimeError, match="set_polarisation_fields"):
        h.load_response()
    h.set_polarisation_fields(S.fields(h))
    plan = h._plan
    _close(_run(h, g), want, 1e-13, f"{kind}: Expression against callable polarisation")
    N, n_el, t = h._msh.num_cells, h._cell_mesh.num_cells, h._tensor_size()
    assert h._plan is plan and plan.load_calls[-1][1:] == ((N, 1, n_el, t), True, False)  # per-cell element means, as of a callable
    r = h.load_response(cells=[1, 4])
    assert r.P_eff.shape == (2, 1, t) and S.difference(r.P_eff[:, 0], want[1][[1, 4]]) < 1e-12
    # other parameters: the same plan, another load
    h.set_polarisation(E.with_parameters([-3.0]) if E.n_params else E)
    again = _run(h, g)
    assert h._plan is plan and (not E.n_params or S.difference(again[1], want[1]) > 1e-3)  # (a load that is constant in x moves P_eff, not u)


@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_eigenstrain_equals_the_host_formed_eigenstress_on_a_stand_in(kind):
    h, E, P, g, Ec = _problem(kind)
    cells = np.arange(h._msh.num_cells)
    h.set_polarisation(Ec)
    means = h._polarisation_loads(cells)[0][:, 0]  # element means of E, [N, n_el, t]
    coef, packed = h._element_means(cells)
    h.set_polarisation(hmm.eigenstress(coef, packed, 2, means))
    want = _run(h, g)
    h.set_eigenstrain(Ec)
    got = _run(h, g)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert h._plan.load_calls[-1][1:] == (means[:, None].shape, True, False)  # the stand-in sees a per-cell load and nothing new
    h.set_eigenstrain(means)
    got = _run(h, g)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    h.set_eigenstrain(means[0])  # shared by all macro cells: the eigenstress is still per cell
    shared = _run(h, g)
    assert h._plan.load_calls[-1][1:] == (means[:, None].shape, True, False) and S.difference(shared[1][0], want[1][0]) < 1e-13
    h.set_eigenstrain(E)
    h.set_polarisation_fields(S.fields(h))
    by_expression = _run(h, g)
    _close(by_expression, want, 1e-13, f"{kind}: Expression eigenstrain against the host-formed eigenstress")
    # what the device tests take their tolerance from: the host interpreter against the callable of -A : E a user wrote by hand
    h.set_polarisation(P)
    _close(by_expression, _run(h, g), S.CPU_DIFFERENCE[kind], f"{kind}: host interpreter against the hand-written eigenstress")
    # one replaces the other; None removes it
    assert not h._eigenstrain
    h.set_eigenstrain(None)
    plain = S.solve(h, g)
    assert h.effective_polarisation is None and S.difference(plain, want[0]) > 1e-6
    with pytest.raises(RuntimeError, match="set_polarisation"):
        h.load_response()


def test_what_a_load_expression_must_be():
    h, E, _, _, _ = _problem("poisson")
    for setter in (h.set_polarisation, h.set_eigenstrain):
        with pytest.raises(ValueError, match="must be a vector of 2 components"):
            setter(Expression("1.0"))
        with pytest.raises(ValueError, match="must be a vector of 2 components"):
            setter(Expression(["1.0", "2.0", "3.0"]))
    with pytest.raises(ValueError, match="E has shape"):
        h.set_eigenstrain(np.zeros((3, 3)))
    he = _problem("elasticity")[0]
    with pytest.raises(ValueError, match=r"reads y\[2\]"):
        he.set_eigenstrain(Expression(["y[2]", "1.0", "2.0"]))


def test_set_polarisation_fields():
    h, E, _, g, _ = _problem("poisson")
    N = h._msh.num_cells
    with pytest.raises(ValueError, match="set_polarisation_fields\\(\\) needs"):
        h.set_polarisation_fields(np.ones(N))
    h.set_polarisation(lambda x, y: [0.0 * y[0]] * 2)
    with pytest.raises(ValueError, match="set_polarisation_fields\\(\\) needs"):
        h.set_polarisation_fields(np.ones(N))
    h.set_polarisation(Expression(["1.0", "y[0]"]))  # an Expression without fields needs none
    with pytest.raises(ValueError, match="set_polarisation_fields\\(\\) needs"):
        h.set_polarisation_fields(np.ones(N))
    S.solve(h, g)
    h.set_eigenstrain(E)
    for bad in (np.ones(N + 1), np.ones((N, 2)), np.ones((2, N))):
        with pytest.raises(ValueError, match="need values of shape"):
            h.set_polarisation_fields(bad)
    for value in (np.nan, np.inf):
        v = np.ones(N)
        v[3] = value
        with pytest.raises(ValueError, match="field dT is not finite on macro cell 3"):
            h.set_polarisation_fields(v)
    assert h._polarisation_fields is None  # nothing a failed call leaves behind
    h.set_polarisation_fields(S.fields(h))  # [N] for one field
    a = _run(h, g)
    h.set_polarisation_fields(S.fields(h)[:, None])  # [N, 1]
    b = _run(h, g)
    h.set_polarisation_fields(lambda x: S.dT(x))  # a callable of the midpoints
    c = _run(h, g)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
    assert h._fields is None  # the coefficient's fields are another matter
    with pytest.raises(ValueError, match="set_fields\\(\\) needs"):
        h.set_fields(np.ones(N))


# -- a plan that takes load sources -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_an_expression_crosses_as_its_program(kind):
    h, E, P, g, Ec = _problem(kind)
    h.set_eigenstrain(E)
    h.set_polarisation_fields(S.fields(h))
    want = _run(h, g)  # the stand-in without the capability
    h._plan = plan = SourcePlan(2, N_MICRO[kind], kind)
    plan.expression = E
    got = _run(h, g)
    N, n_el, t = h._msh.num_cells, h._cell_mesh.num_cells, h._tensor_size()
    (given, per_cell, kw), = plan.given
    assert isinstance(given, CoefStream) and given.method == "solve_program" and per_cell is None and kw == {"eigenstrain": True}
    assert given.per_cell.shape == (N, 4) and np.array_equal(given.per_cell[:, 3], S.fields(h))  # the midpoint, then dT: what crosses per cell
    assert np.array_equal(given.per_cell[:, :3], h._msh.cell_midpoints())
    yq, w = h._quadrature_points()
    assert np.array_equal(given.shared[0], yq) and np.array_equal(given.shared[1], w)  # the points that sample the coefficient
    _close(got, want, 1e-13, f"{kind}: the program path against the element means")
    # a polarisation: the same stream without the flag
    h.set_polarisation(E)
    _run(h, g)
    given, per_cell, kw = plan.given[-1]
    assert isinstance(given, CoefStream) and per_cell is None and kw == {}
    # load_response sends the stream too, chunk by chunk with the rows of the chunk
    h.load_response(cells=[5, 2, 7], chunk_cells=2)
    assert [len(c[0]) for c in plan.given[-2:]] == [2, 1] and all(isinstance(c[0], CoefStream) for c in plan.given[-2:])
    assert np.array_equal(plan.given[-2][0].per_cell[:, 3], S.fields(h)[[5, 2]]) and plan.given[-2][2] == {"response": True, "fields": False, "return_correctors": False}
    # an eigenstrain given as a callable or an array crosses as E, and the plan forms the eigenstress
    h.set_eigenstrain(Ec)
    by_callable = _run(h, g)
    given, per_cell, kw = plan.given[-1]
    assert isinstance(given, np.ndarray) and given.shape == (N, 1, n_el, t) and per_cell is True and kw == {"eigenstrain": True}
    _close(by_callable, want, 1e-13, f"{kind}: E as a callable on a plan that forms the eigenstress")
    h.set_eigenstrain(given[0, 0])
    _run(h, g)
    given, per_cell, kw = plan.given[-1]
    assert given.shape == (1, n_el, t) and per_cell is False and kw == {"eigenstrain": True}


@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
@pytest.mark.parametrize("plan", [LoadOraclePlan, SourcePlan])
def test_array_and_callable_polarisations_send_the_calls_they_sent(kind, plan):
    h, E, P, g, Ec = _problem(kind, plan)
    N, n_el, t = h._msh.num_cells, h._cell_mesh.num_cells, h._tensor_size()
    h.set_polarisation(P)
    with_P = _run(h, g)
    assert h._plan.load_calls == [((N, n_el) + (() if kind == "poisson" else (2,)), (N, 1, n_el, t), True, False)]
    means = h._polarisation_loads(np.arange(N))[0][:, 0]
    h.set_polarisation(means)
    assert np.array_equal(_run(h, g)[0], with_P[0]) and h._plan.load_calls[-1][1:] == ((N, 1, n_el, t), True, False)
    h.set_polarisation(means[0])
    _run(h, g)
    assert h._plan.load_calls[-1][1:] == ((1, n_el, t), False, False)
    if plan is SourcePlan:  # no keyword the earlier interface does not have
        assert all(kw == {} and isinstance(given, np.ndarray) for given, _, kw in h._plan.given)
