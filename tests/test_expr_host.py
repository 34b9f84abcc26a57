"""Expression coefficients on the CPU: the grammar, the degree estimate, the limits of the program, the NumPy interpreter against plain
lambdas, ``host_stream`` against the tensordot of the samples, and the solver classes on stub plans -- an ``Expression`` reaches a plan
that has ``solve_program`` as its CoefStream without ever being sampled on the host, a plan without it gets element means, and the
quadrature degree is the expression's own (no heuristic, no warning).  No GPU needed."""

import logging

import numpy as np
import pytest

from hommx_amd import expr, hmm, mesh
from hommx_amd.batch import CoefStream, Program

E = hmm.Expression
SMOOTH = "1.1 + x[0] + sin(2*pi*y[0])"


# -- grammar ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [
    "y.real", "np.sin(y[0])",                 # attribute access
    "z", "e + 1", "x",                        # unknown names (x and y only indexed)
    "sinh(y[0])", "eval('1')", "sin(y[0], 2)",  # unknown calls / arity
    "y[0]**x[0]", "y[0]**2.0", "y[0]**9", "y[0]**-1",  # the exponent is a literal integer 0 .. 8
    "'abc'", "y[0] + 'a'",                    # string literals
    "x[3]", "y[-1]", "y[x[0]]",               # indices
    "y[0] < 1", "where(y[0], 1, 2)", "1 + (y[0] < 1)", "(y[0] < 1) < 2", "0 < y[0] < 1",  # comparisons are conditions only
    "y[0] if x[0] else 1", "[1, 2]", "lambda: 1", "y[0] % 2", "True", "1 +",
])
def test_outside_the_grammar_raises(text):
    with pytest.raises(ValueError, match="expression"):
        E(text)


def test_constructor_forms():
    assert E("1").shape == "scalar" and E(lam="1", mu="2").shape == "lame" and E(lam="1", mu="2").n_comp == 2
    m = E([["1 + y[0]", "x[0] * y[1]"], ["x[0]*y[1]", "2"]])  # equal trees, whatever the spacing
    assert m.shape == "matrix" and m.dim == 2 and m.n_comp == 3
    assert E([["1", "0", "0"], ["0", "1", "y[2]"], ["0", "y[2]", "1"]]).n_comp == 6
    with pytest.raises(ValueError, match="symmetric"):
        E([["1", "y[0]"], ["y[1]", "1"]])
    with pytest.raises(ValueError, match="symmetric"):
        E([["1", "y[0] + 1"], ["1 + y[0]", "1"]])  # equal values, different trees
    for bad in (dict(lam="1"), dict(text="1", lam="1", mu="2"), dict()):
        with pytest.raises(ValueError):
            E(**bad)
    with pytest.raises(ValueError):
        E([["1", "2", "3"], ["2", "1", "3"]])


# -- degrees ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,degree", [
    (SMOOTH, 3), ("1/(2 + cos(2*pi*y[0]))", 3), ("where(y[0] < 0.5, 1, 100)", 0), ("y[0]*y[1]", 2), ("sin(x[0])", 0),
    ("3.5", 0), ("pi*x[1]", 0), ("y[0]", 1), ("y[0] - y[1]**2", 2), ("y[0]**3/y[1]", 4), ("abs(y[0] - 0.5)", 1), ("(1 + y[0])**0", 0),
    ("min(y[0], y[1]*y[1])", 2), ("max(1, x[0])", 0), ("where(y[0]*y[0]*y[0] < 0.1, y[1], 2)", 1), ("sin(y[0])*cos(y[1])", 6),
    ("exp(y[0]*y[1])", 4), ("sqrt(2)", 0), ("-y[0]", 1), ("1 + 0.9*sin(2*pi*y[0])*cos(x[0]*y[1])", 6),
])
def test_degree_follows_the_tree(text, degree):
    assert E(text).degree == degree


def test_degree_of_several_components_is_the_largest():
    assert E(lam="1.25", mu="5 + 4.5*sin(2*pi*y[0])").degree == 3
    assert E([["1", "y[0]*y[1]"], ["y[0]*y[1]", "y[0]"]]).degree == 2


# -- the program ----------------------------------------------------------------------------------------------------------------------
def test_program_is_postfix_with_one_store_per_component():
    ops, consts = E(lam="1.25", mu="5 + 4.5*y[0]").program()
    assert ops.dtype == np.uint8 and ops.shape[1] == 2 and consts.dtype == np.float64
    stores = [int(k) for op, k in ops if op == expr.OP_STORE]
    assert stores == [0, 1] and ops[-1, 0] == expr.OP_STORE
    assert expr.stack_depths(ops.tolist())[-1] == 0


def test_literals_fold_where_python_brings_them_together():
    ops, consts = E("2*pi*y[0]").program()  # (2 * pi) * y[0]
    assert list(consts) == [2 * np.pi] and [int(o) for o in ops[:, 0]] == [expr.OP_CONST, expr.OP_Y, expr.OP_MUL, expr.OP_STORE]
    ops, consts = E("y[0]*2*pi").program()  # (y[0] * 2) * pi: nothing to fold
    assert list(consts) == [2.0, np.pi] and len(ops) == 6
    ops, consts = E("sin(pi/6) + y[0]").program()
    assert list(consts) == [np.sin(np.pi / 6)]
    ops, consts = E("2 + y[0] + 2").program()  # equal constants share a slot
    assert list(consts) == [2.0]


def test_power_is_a_chain_of_multiplications():
    ops, _ = E("y[0]**4").program()
    assert [int(o) for o in ops[:, 0]] == [expr.OP_Y] + [expr.OP_DUP] * 3 + [expr.OP_MUL] * 3 + [expr.OP_STORE]
    assert [int(o) for o in E("y[0]**1").program()[0][:, 0]] == [expr.OP_Y, expr.OP_STORE]


def test_program_limits():
    deep = "y[0]"
    for _ in range(expr.MAX_STACK):
        deep = f"y[0] + ({deep})"  # right-nested: one more value waits on the stack per level
    with pytest.raises(ValueError, match="too deep"):
        E(deep)
    E("y[0] + (" * (expr.MAX_STACK - 1) + "y[0]" + ")" * (expr.MAX_STACK - 1))  # depth 16 exactly
    with pytest.raises(ValueError, match="too long"):
        E(" + ".join(["y[0]*y[1]"] * 40))
    with pytest.raises(ValueError, match="too many constants"):
        E("y[0]" + "".join(f" + {k}.5" for k in range(expr.MAX_CONSTS + 1)))  # (y[0] + 0.5) + 1.5 ...: no two literals meet
    assert len(E("y[0]" + "".join(f" + {k}.5" for k in range(expr.MAX_CONSTS))).program()[1]) == expr.MAX_CONSTS
    with pytest.raises(ValueError, match="underflow"):
        expr.stack_depths([(expr.OP_Y, 0), (expr.OP_ADD, 0)])


# -- host evaluation ------------------------------------------------------------------------------------------------------------------
RNG = np.random.default_rng(7)
X, Y = RNG.uniform(-1, 2, (3, 6, 1)), RNG.uniform(0, 1, (3, 1, 41))

EXACT = [
    ("1.1 + x[0] + y[0]*x[1] - y[1]/3", lambda x, y: 1.1 + x[0] + y[0] * x[1] - y[1] / 3),
    ("-(y[0] - 0.5)/(2 + x[2]*y[1])", lambda x, y: -(y[0] - 0.5) / (2 + x[2] * y[1])),
    ("abs(y[0] - 0.5) + min(y[0], y[1]) - max(x[0], y[2])", lambda x, y: np.abs(y[0] - 0.5) + np.minimum(y[0], y[1]) - np.maximum(x[0], y[2])),
    ("where(abs(y[0] - 0.5) < 0.25 and y[1] >= x[0], 10*x[1], 1 + y[2])",
     lambda x, y: np.where((np.abs(y[0] - 0.5) < 0.25) & (y[1] >= x[0]), 10 * x[1], 1 + y[2])),
    ("where(not y[0] <= 0.3 or y[1] > 0.9, 2, 3)", lambda x, y: np.where(~(y[0] <= 0.3) | (y[1] > 0.9), 2.0, 3.0)),
    ("2*pi*y[0] + y[1]*2*pi", lambda x, y: 2 * np.pi * y[0] + y[1] * 2 * np.pi),
    ("3", lambda x, y: np.full(np.broadcast(x[0], y[0]).shape, 3.0)),
]


@pytest.mark.parametrize("text,fn", EXACT)
def test_exact_operations_equal_the_lambda_bitwise(text, fn):
    got = E(text)(X, Y)
    assert got.shape == (6, 41) and np.array_equal(got, np.broadcast_to(fn(X, Y), (6, 41)))


def test_integer_powers_are_products():
    a = Y[0] + X[1]
    assert np.array_equal(E("(y[0] + x[1])**3")(X, Y), a * a * a)
    assert np.array_equal(E("(y[0] + x[1])**8")(X, Y), ((((((a * a) * a) * a) * a) * a) * a) * a)
    assert np.array_equal(E("(y[0] + x[1])**0 + y[0]")(X, Y), 1.0 + Y[0] + 0 * X[0])


def test_functions_are_numpys():
    for name, fn in (("sqrt", np.sqrt), ("sin", np.sin), ("cos", np.cos), ("tan", np.tan), ("exp", np.exp), ("log", np.log), ("tanh", np.tanh)):
        assert np.array_equal(E(f"2 + {name}(1 + y[0]*x[0]*x[0])")(X, Y), 2 + fn(1 + Y[0] * X[0] * X[0])), name


def test_components_and_point_calls():
    v = E(lam="1.25", mu="5 + 4.5*y[0]")(X, Y)
    assert isinstance(v, hmm.Lame) and np.array_equal(v.mu, 5 + 4.5 * Y[0] + 0 * X[0]) and np.all(v.lam == 1.25) and v.lam.shape == (6, 41)
    m = E([["1 + y[0]", "x[0]*y[1]"], ["x[0]*y[1]", "2"]])(X, Y)
    assert m.shape == (6, 41, 2, 2) and np.array_equal(m[..., 0, 1], X[0] * Y[1]) and np.array_equal(m[..., 1, 0], m[..., 0, 1])
    assert np.all(m[..., 1, 1] == 2.0)
    # the per-cell call of the solver classes: x[3], y[d, npts]
    assert np.array_equal(E(SMOOTH)(X[:, 2, 0], Y[:2, 0]), 1.1 + X[0, 2, 0] + np.sin(2 * np.pi * Y[0, 0]))
    with pytest.raises(ValueError, match=r"y\[2\]"):
        E("y[2]")(X, Y[:2])


# -- host_stream ----------------------------------------------------------------------------------------------------------------------
def solver(A, cls=hmm.PoissonHMM, nx=3, n=4, **kw):
    f = (lambda x: 1.0) if cls is hmm.PoissonHMM else (lambda x: np.array([0.0, -1.0]))
    return cls(mesh.create_unit_square(nx, nx), A, f, mesh.create_unit_square(n, n), 0.01, **kw)


@pytest.mark.parametrize("A,fn", [
    (E(SMOOTH), lambda x, y: 1.1 + x[0] + np.sin(2 * np.pi * y[0])),
    (E("where(y[0] < 0.5, 1 + x[1], 100)"), lambda x, y: np.where(y[0] < 0.5, 1 + x[1], 100.0)),
    (E("1 + y[0]*y[1]"), lambda x, y: 1 + y[0] * y[1]),
])
def test_host_stream_is_the_tensordot_of_the_samples(A, fn):
    h = solver(A)
    yq, w = h._quadrature_points()
    assert yq.shape[1] == {0: 1, 2: 3, 3: 6}[A.degree]
    c = h._msh.cell_midpoints()
    got = A.host_stream(c, yq, w)
    v = np.broadcast_to(fn(c.T[:, :, None, None], np.moveaxis(yq, -1, 0)[:, None]), (len(c),) + yq.shape[:2])  # [N, n_el, n_q]
    assert got.shape == v.shape[:2] and np.allclose(got, np.tensordot(v, w, axes=([2], [0])), rtol=1e-14, atol=0)  # _sample_batched's own check
    lam = E(lam="2", mu=SMOOTH).host_stream(c, yq, w)
    assert lam.shape == got.shape + (2,) and np.all(np.abs(lam[..., 0] - 2.0) < 1e-15)
    if A.texts[0] == SMOOTH:
        assert np.array_equal(lam[..., 1], got)


# -- solver classes on stub plans -------------------------------------------------------------------------------------------------------
class MeansPlan:
    """A stand-in that takes element means only."""

    def __init__(self, kind="poisson", t=2):
        self.kind, self.t, self.seen = kind, t, []

    def solve(self, coef, M=None, return_info=False):
        self.seen.append(coef)
        out = np.tile(np.eye(self.t), (len(coef), 1, 1))
        return (out, np.zeros(len(coef), np.int32)) if return_info else out


class ProgramPlan(MeansPlan):
    """... and one that offers the method of the program form."""

    def solve_program(self, points, weights, program, midpoints, M=None, return_info=False):
        self.seen.append(CoefStream("solve_program", (points, weights, program), midpoints))
        return self.solve(np.ones((len(midpoints), len(points))), M, return_info)


def test_expression_reaches_the_plan_as_its_stream(monkeypatch):
    A = E(SMOOTH)
    h = solver(A)
    h._plan = ProgramPlan()

    def no_means(self, cells, coeff=None):
        raise AssertionError("a device-sampled coefficient must not be sampled on the host")

    monkeypatch.setattr(hmm.BaseHMM, "_element_means", no_means)
    h.solve()
    stream = h._plan.seen[0]
    assert isinstance(stream, CoefStream) and stream.method == "solve_program"
    points, weights, prog = stream.shared
    assert points.shape == (32, 6, 2) and weights.shape == (6,) and isinstance(prog, Program) and prog.n_comp == 1
    assert np.array_equal(prog.ops, A.program()[0]) and np.array_equal(prog.consts, A.program()[1])
    assert np.array_equal(stream.per_cell, h._msh.cell_midpoints()) and stream.per_cell.shape == (18, 3)
    src = stream.coef_source()
    assert (src.form, src.n_q, src.table, src.weights, src.params) == (3, 6, points.ctypes.data, weights.ctypes.data, stream.per_cell.ctypes.data)
    g = src.program.contents
    assert (g.n_ops, g.n_consts, g.n_comp, g.ops, g.consts) == (len(prog.ops), 2, 1, prog.ops.ctypes.data, prog.consts.ctypes.data)
    src = stream.coef_source(address=lambda a: 4096)  # an upload: the program stays host memory
    assert (src.table, src.weights, src.params, src.program.contents.ops) == (4096, 4096, 4096, prog.ops.ctypes.data)


def test_stand_in_without_the_method_gets_element_means():
    A = E(SMOOTH)
    h = solver(A)
    h._plan = MeansPlan()
    h.solve()
    (coef,) = h._plan.seen
    yq, w = h._quadrature_points()
    assert isinstance(coef, np.ndarray) and coef.shape == (18, 32)
    assert np.allclose(coef, A.host_stream(h._msh.cell_midpoints(), yq, w), rtol=1e-14, atol=0)


@pytest.mark.parametrize("text", [SMOOTH, "where(y[0] < 0.5, 1, 100)", "1 + y[0]*y[1]", "1 + 0.9*sin(2*pi*y[0])*cos(x[0]*y[1])"])
def test_quadrature_degree_is_the_expressions_own(caplog, text):
    A = E(text)
    with caplog.at_level(logging.DEBUG):
        h = solver(A)
        h._plan = ProgramPlan()
        assert h.quadrature_degree_used == A.degree
        h.solve()
    assert h.quadrature_degree_used == A.degree
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    g = solver(A, quadrature_degree=2)  # an explicit integer still overrides
    g._plan = ProgramPlan()
    g.solve()
    assert g.quadrature_degree_used == 2 and g._plan.seen[0].shared[0].shape[1] == 3


def test_heuristic_never_runs_for_an_expression(monkeypatch):
    def boom(self, *a):
        raise AssertionError("the sampling heuristic must not run for an Expression")

    monkeypatch.setattr(hmm.BaseHMM, "_auto_quadrature_degree", boom)
    for plan in (ProgramPlan(), MeansPlan()):
        h = solver(E("where(y[0] < 0.5, 1, 100)"))
        h._plan = plan
        h.solve()


def test_shapes_must_fit_the_class():
    lame, matrix = E(lam="1", mu="2"), E([["1", "0"], ["0", "1"]])
    h = solver(lame)
    h._plan = ProgramPlan()
    with pytest.raises(ValueError, match="scalar or a symmetric 2 x 2 matrix"):
        h.solve()
    for bad in (E("1"), matrix):
        g = solver(bad, hmm.LinearElasticityHMM)
        g._plan = ProgramPlan("elasticity", 3)
        with pytest.raises(ValueError, match="lam="):
            g.solve()
    h = solver(E([["1", "0", "0"], ["0", "1", "0"], ["0", "0", "1"]]))
    h._plan = ProgramPlan()
    with pytest.raises(ValueError, match="2 x 2"):
        h.solve()
    h = solver(E("1 + y[2]"))
    h._plan = ProgramPlan()
    with pytest.raises(ValueError, match=r"y\[2\]"):
        h.solve()
    # the forms that fit: their plan kinds
    assert solver(matrix)._micro_kind() == "poisson_matrix" and solver(E("1"))._micro_kind() == "poisson"
    g = solver(lame, hmm.LinearElasticityHMM)
    g._plan = ProgramPlan("elasticity", 3)
    g.solve()
    assert g._plan.seen[0].shared[2].n_comp == 2


def test_parameter_derivatives_stay_out_of_scope():
    h = solver(E(SMOOTH))
    h._plan = ProgramPlan()
    with pytest.raises(ValueError, match="no parameters"):
        h.tensor_derivatives()
