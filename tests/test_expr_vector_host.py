"""The vector shape of an ``Expression`` -- a flat list of 1 to 6 texts, the form of a polarisation or an eigenstrain -- on the CPU: it
parses, has the shape, degree and call of its components, and every component of its streams is bit for bit the stream of the scalar
expression of that text; the solver classes go on refusing it as a coefficient."""

import numpy as np
import pytest

from hommx_amd import hmm, mesh
from hommx_amd.expr import Expression

TEXTS = ["p[0]*y[0] + f[0]", "sin(2*pi*y[1])*x[0] - p[1]", "where(y[0] < 0.5, f[1], 2.0)*y[0]*y[1]", "1.5", "exp(-f[0]*y[0])/(1 + p[0]**2)",
         "y[0]*y[0]*y[0]"]
KW = dict(p=[0.7, -1.3], fields=("dT", "c"))


def _points(dim=2, n_el=7, nq=3, n=4, seed=0):
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.5, 2, (n, 2))], axis=1)
    return rows, rng.uniform(0, 1, (n_el, nq, dim)), rng.uniform(0.1, 1, nq)


@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_a_flat_list_is_a_vector(n):
    e = Expression(TEXTS[:n], **KW)
    assert e.shape == "vector" and e.n_comp == n and e.dim is None
    assert e.degree == max(Expression(t, **KW).degree for t in TEXTS[:n])
    assert (e.n_params, e.n_fields, e.field_names) == (2, 2, ("dT", "c"))
    ops, consts = e.program()
    assert [k for op, k in ops.tolist() if op == 27] == list(range(n))  # one STORE per component, in order
    assert np.array_equal(consts[:2], KW["p"])
    rows, yq, w = _points()
    v = e(rows.T[:, :, None], np.moveaxis(yq[:, 0, :], -1, 0)[:, None, :])
    assert isinstance(v, np.ndarray) and v.shape == (n, 4, 7)  # [n_comp, ...]: what set_polarisation documents for a callable
    assert Expression(tuple(TEXTS[:n]), **KW).shape == "vector"
    other = e.with_parameters([2.0, 3.0])
    assert other.shape == "vector" and np.array_equal(other.p, [2.0, 3.0]) and np.array_equal(e.p, KW["p"])


@pytest.mark.parametrize("n", [1, 2, 6])
def test_every_component_is_the_scalar_expression_bitwise(n):
    e = Expression(TEXTS[:n], **KW)
    rows, yq, w = _points()
    stream, tangents = e.host_stream(rows, yq, w), e.host_tangents(rows, yq, w)
    assert stream.shape == (4, 7, n) and tangents.shape == (4, 4, 7, n)  # the component axis stays, whatever n is
    x, y = rows.T[:, :, None], np.moveaxis(yq[:, 1, :], -1, 0)[:, None, :]
    for c, text in enumerate(TEXTS[:n]):
        s = Expression(text, **KW)
        assert np.array_equal(stream[..., c], s.host_stream(rows, yq, w))
        assert np.array_equal(tangents[..., c], s.host_tangents(rows, yq, w))
        assert np.array_equal(e.components(x, y)[c], s.components(x, y)[0])


def test_what_is_no_vector_raises():
    for bad in ([], ["1.0"] * 7, ["1.0", ["2.0", "3.0"]], [["1.0", "2.0"], "3.0"]):
        with pytest.raises(ValueError):
            Expression(bad)
    assert Expression([["1.0", "y[0]"], ["y[0]", "2.0"]]).shape == "matrix"  # a nested list stays a matrix
    with pytest.raises(ValueError, match="unknown name"):
        Expression(["1.0", "z"])


def test_the_solver_classes_refuse_it_as_a_coefficient():
    msh, cell = mesh.create_unit_square(2, 2), mesh.create_unit_square(4, 4)
    h = hmm.PoissonHMM(msh, Expression(["1.0", "2.0"]), lambda x: 1.0 + x[0], cell, 0.01)
    with pytest.raises(ValueError, match="must be a scalar or a symmetric 2 x 2 matrix; got a vector"):
        h._device_form()
    e = hmm.LinearElasticityHMM(msh, Expression(["1.0", "2.0", "3.0"]), lambda x: np.array([0.0, -1.0]), cell, 0.01)
    with pytest.raises(ValueError, match=r"must be Expression\(lam=..., mu=...\); got a vector"):
        e._device_form()
