"""Parameters ``p[k]`` of an ``Expression`` on the CPU: the grammar and what it emits, the degree in the parameters, the tangent rules of
``host_tangents`` (include/hommx_hip.h, hommx_expand_tangents) against closed-form derivatives written as expressions of their own, the
zero-tangent rule, and the validation of n_params and of HOMMX_DIRS_PARAMETERS at the C ABI, which runs on the host before the plan's
device is made current (the manner of test_program_abi_host.py).  No GPU needed."""

import ctypes as C
import logging
import os

import numpy as np
import pytest

from hommx_amd import _lib, expr
from hommx_amd.batch import CoefStream, Program
from hommx_amd.expr import Expression as E
from test_program_abi_host import GOOD, P as PTR, call, source
from test_reconstruct_source_host import _fake_plan


# -- 1. grammar and emission -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,kw,message", [
    ("1 + p[0]", {}, "p[k] needs the values of the parameters (p=[...]): Subscript 'p[0]'"),
    ("1 + p[1]", dict(p=[1.0]), "the index of p is a literal integer below the number of parameters (1): Subscript 'p[1]'"),
    ("1 + p[-1]", dict(p=[1.0]), "the index of p is a literal integer below the number of parameters (1): Subscript 'p[-1]'"),
    ("1 + p[x[0]]", dict(p=[1.0]), "the index of p is a literal integer below the number of parameters (1): Subscript 'p[x[0]]'"),
    ("1 + p[0]", dict(p=[1, 2, 3, 4, 5]), "at most 4 parameters; got 5"),
    ("1 + p[0]", dict(p=[float("inf")]), "parameter p[0] is not finite: inf"),
    ("1 + p[0]", dict(p=[1.0, float("nan")]), "parameter p[1] is not finite: nan"),
    ("1 + p[0]", dict(p=[1.0], parameter_names=("a", "b")), "2 parameter_names for 1 parameters"),
    ("1 + p", dict(p=[1.0]), "unknown name"),
])
def test_errors_name_the_fault(text, kw, message):
    with pytest.raises(ValueError) as e:
        E(text, **kw)
    assert str(e.value).startswith("expression: ") and message in str(e.value)


def test_parameters_are_the_first_constants_and_nothing_folds_into_them():
    p = [0.1, 2.0, 0.1, -3.5]  # one of them unused, two of them equal, one equal to a literal of the text
    A = E("2.0*p[0] + p[3]*y[0] + 0.1 + p[2]", p=p)
    ops, consts = A.program()
    assert A.n_params == 4 and A.parameter_names == ("p0", "p1", "p2", "p3")
    assert consts[:4].tobytes() == np.array(p).tobytes() and A.p.tobytes() == np.array(p).tobytes()
    A.p[0] = 7.0  # a copy
    assert A.p[0] == 0.1
    used = [int(k) for op, k in ops if op == expr.OP_CONST]
    assert used == [4, 0, 3, 5, 2]  # the literals 2.0 and 0.1 have slots of their own; p[2] keeps its slot beside its equal p[0]
    assert consts[4] == 2.0 and consts[5] == 0.1 and len(consts) == 6
    assert [int(op) for op, _ in ops].count(expr.OP_MUL) == 2  # "2.0*p[0]" holds a MUL
    ops2, consts2 = E("2*p[0]", p=[3.0]).program()
    assert ops2.tolist() == [[expr.OP_CONST, 1], [expr.OP_CONST, 0], [expr.OP_MUL, 0], [expr.OP_STORE, 0]] and consts2.tolist() == [3.0, 2.0]
    assert E("2*pi*y[0] + p[0]", p=[1.0]).program()[1].tolist() == [1.0, 2 * np.pi]  # literals still fold among themselves
    assert E("y[0]", p=[1.0, 2.0]).program()[1].tolist() == [1.0, 2.0] and E("y[0]", p=[]).n_params == 0
    assert E("y[0]").n_params == 0 and E("y[0]").p.size == 0 and E("y[0]").parameter_names == ()


def test_the_constants_limit_counts_the_parameters():
    text = " + ".join(f"{k + 2}.5*y[0]" for k in range(expr.MAX_CONSTS - 1))  # 31 distinct literals
    assert len(E(text, p=[1.0]).program()[1]) == expr.MAX_CONSTS
    with pytest.raises(ValueError, match="too many constants: 33"):
        E(text, p=[1.0, 2.0])


def test_with_parameters_keeps_the_program():
    A = E(lam="1.25 + p[1]*x[0]", mu="5 + p[0]*sin(2*pi*y[0])", p=[4.5, 0.5], parameter_names=("amplitude", "slope"))
    B = A.with_parameters([1.0, 2.0])
    assert B is not A and B.parameter_names == ("amplitude", "slope") and B.n_params == 2 and B.shape == "lame"
    assert np.array_equal(A.program()[0], B.program()[0])
    assert B.program()[1][:2].tolist() == [1.0, 2.0] and np.array_equal(A.program()[1][2:], B.program()[1][2:])
    assert A.p.tolist() == [4.5, 0.5]  # the original is untouched
    x, y = np.zeros((3, 1)), np.array([[0.25], [0.5]])
    assert B(x, y).mu[0] == 5 + np.sin(2 * np.pi * 0.25) and A(x, y).mu[0] == 5 + 4.5 * np.sin(2 * np.pi * 0.25)
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, float("inf")]):
        with pytest.raises(ValueError, match="expression: "):
            A.with_parameters(bad)
    with pytest.raises(ValueError):
        E("y[0]").host_tangents(np.zeros((1, 3)), np.zeros((1, 1, 2)), np.ones(1))


P_DEGREE = [
    ("1 + x[0]*y[0]", 0), ("p[0]", 1), ("2*p[0] + p[1]*sin(2*pi*y[0])", 1), ("p[0]*p[1]", 2), ("(p[0] + y[0])**3", 3), ("p[0]**0", 0),
    ("p[0]/(1 + y[0])", 1), ("1/(1 + p[0])", np.inf), ("tanh(p[0]*(y[0] - 0.5))", np.inf), ("abs(p[0])", np.inf), ("min(p[0], 1)", np.inf),
    ("max(y[0], 0.5)*p[1]", 1), ("where(y[0] < 0.5, p[1], p[0]*p[0])", 2), ("-p[0] - p[1]", 1),
]


@pytest.mark.parametrize("text,degree", P_DEGREE)
def test_degree_in_the_parameters(text, degree, caplog):
    with caplog.at_level(logging.WARNING):
        A = E(text, p=[0.5, 0.25])
    assert A.p_degree == degree and A.affine_in_parameters == (degree <= 1)
    assert not caplog.records


def test_a_parameter_inside_a_comparison_warns_once(caplog):
    with caplog.at_level(logging.WARNING):
        A = E([["where(y[0] < p[0], 2, 1)", "0"], ["0", "where(y[1] < p[0] or y[0] > 0.5, 2, 1)"]], p=[0.5])
    assert A.p_degree == 0 and A.affine_in_parameters  # the condition does not count
    warnings = [r for r in caplog.records if r.levelname == "WARNING"]
    assert len(warnings) == 1 and "inside a comparison" in warnings[0].getMessage() and "y[0] < p[0]" in warnings[0].getMessage()
    yq = np.array([[[0.25, 0.5]], [[0.75, 0.5]]])
    assert not A.host_tangents(np.zeros((1, 3)), yq, np.ones(1)).any()  # zero almost everywhere: the motion of the interface is ignored


# -- 2. the rules, exact family ----------------------------------------------------------------------------------------------------------
# Points, midpoints, weights and parameters are small dyadic rationals and the texts have low degree, so no operation rounds: the
# tangents must equal the closed-form derivative, whatever the order of its operations.  (text, derivatives, a condition both of whose
# outcomes must occur or None)
EXACT_P = [0.5, 1.5]
EXACT = [
    ("p[0]*y[0] + p[1]*x[0] - p[0]", ["y[0] - 1", "x[0]"], None),  # ADD SUB MUL
    ("-(p[0]*y[1]) + x[1]*p[1]*p[1]", ["-y[1]", "2*x[1]*p[1]"], None),  # NEG, a product of parameters
    ("abs(p[0]*(y[0] - 0.5))", ["where(p[0]*(y[0] - 0.5) < 0, 0.5 - y[0], y[0] - 0.5)", "0"], "y[0] < 0.5"),
    ("min(p[0]*y[0], y[1])", ["where(y[1] < p[0]*y[0], 0, y[0])", "0"], "y[1] < p[0]*y[0]"),
    ("max(p[0]*y[0], p[1]*y[1])", ["where(p[1]*y[1] > p[0]*y[0], 0, y[0])", "where(p[1]*y[1] > p[0]*y[0], y[1], 0)"], "p[1]*y[1] > p[0]*y[0]"),
    ("where(y[0] < 0.5, p[0]*y[1], p[1]*x[0])", ["where(y[0] < 0.5, y[1], 0)", "where(y[0] < 0.5, 0, x[0])"], "y[0] < 0.5"),
    ("(p[0] + y[0])**3", ["3*(p[0] + y[0])**2", "0"], None),  # DUP
    ("(p[0]*y[0] + y[1])/4 + p[1]/8", ["y[0]/4", "0.125"], None),  # DIV by a power of two
]


def _dyadic_case():
    rng = np.random.default_rng(7)
    x = rng.integers(0, 9, (5, 3)) / 8.0
    yq = rng.integers(0, 17, (11, 2, 2)) / 16.0
    return x, yq, np.array([0.25, 0.75])


@pytest.mark.parametrize("text,derivatives,condition", EXACT, ids=[c[0] for c in EXACT])
def test_exact_rules_equal_the_closed_form_bitwise(text, derivatives, condition):
    x, yq, w = _dyadic_case()
    A = E(text, p=EXACT_P)
    got = A.host_tangents(x, yq, w)
    assert got.shape == (5, 2, 11) and np.all(np.isfinite(got))
    for j, d in enumerate(derivatives):
        want = np.broadcast_to(E(d, p=EXACT_P).host_stream(x, yq, w), (5, 11))
        assert np.array_equal(got[:, j], want), (j, d)
    if condition is not None:  # both branches are hit
        c = np.broadcast_to(E(f"where({condition}, 1, 0)", p=EXACT_P).components(x.T[:, :, None, None], np.moveaxis(yq, -1, 0)[:, None])[0], (5, 11, 2))
        assert c.min() == 0.0 and c.max() == 1.0


def test_exact_rules_on_several_components():
    x, yq, w = _dyadic_case()
    A = E([["1 + p[0]*y[0]", "p[1]*x[0]"], ["p[1]*x[0]", "2 + p[0]*p[1]*y[1]"]], p=EXACT_P)
    got = A.host_tangents(x, yq, w)
    assert got.shape == (5, 2, 11, 3)  # components in the order of the ABI: (0, 0), (1, 1), (0, 1)
    want = [["y[0]", "1.5*y[1]", "0"], ["0", "0.5*y[1]", "x[0]"]]
    for j in range(2):
        for c in range(3):
            assert np.array_equal(got[:, j, :, c], np.broadcast_to(E(want[j][c]).host_stream(x, yq, w), (5, 11))), (j, c)


# -- 3. the rules, rounded family ----------------------------------------------------------------------------------------------------------
# Each closed form is written so that its operations are the rule's, one for one (d(p[0]*u) is add(mul(p[0], 0), mul(1, u)) = u exactly,
# and add(0, -z) = -z), hence equality is bitwise although every operation rounds: no tolerance is needed.
U = "(y[0] - 0.25*x[0])"
ROUNDED = [
    ("div", f"y[1]/(1 + p[0]*{U})", f"-(y[1]/(1 + p[0]*{U})*{U})/(1 + p[0]*{U})"),  # div(add(0, -mul(v, db)), b)
    ("div numerator", f"p[0]/(1 + p[0]*{U})", f"(1 - p[0]/(1 + p[0]*{U})*{U})/(1 + p[0]*{U})"),  # div(add(1, -mul(v, db)), b)
    ("sqrt", f"sqrt(1 + p[0]*{U})", f"{U}/(2*sqrt(1 + p[0]*{U}))"),  # div(da, mul(2, v))
    ("sin", f"sin(p[0]*{U})", f"cos(p[0]*{U})*{U}"),  # mul(cos(a), da)
    ("cos", f"cos(p[0]*{U})", f"-(sin(p[0]*{U})*{U})"),  # -mul(sin(a), da)
    ("tan", f"tan(p[0]*{U})", f"{U}*(1 + tan(p[0]*{U})**2)"),  # mul(da, add(1, mul(v, v)))
    ("exp", f"exp(p[0]*{U})", f"exp(p[0]*{U})*{U}"),  # mul(v, da)
    ("log", f"log(1 + p[0]*{U})", f"{U}/(1 + p[0]*{U})"),  # div(da, a)
    ("tanh", f"tanh(p[0]*{U})", f"{U}*(1 - tanh(p[0]*{U})**2)"),  # mul(da, add(1, -mul(v, v)))
]


@pytest.mark.parametrize("name,text,derivative", ROUNDED, ids=[c[0] for c in ROUNDED])
def test_rounded_rules_equal_the_closed_form_bitwise(name, text, derivative):
    rng = np.random.default_rng(11)
    x, yq = rng.uniform(0.0, 1.0, (4, 3)), rng.uniform(0.0, 1.0, (9, 1, 2))
    w = np.ones(1)  # one point of weight 1: the sum adds nothing to the rule under test
    p = [0.7]
    got = E(text, p=p).host_tangents(x, yq, w)[:, 0]
    want = E(derivative, p=p).host_stream(x, yq, w)
    assert np.all(np.isfinite(want)) and np.abs(want).max() > 0.1
    assert np.array_equal(got, want)
    h = 2.0**-20  # and the closed form is the derivative: a central difference, O(h^2) + O(eps / h)
    fd = (E(text, p=[p[0] + h]).host_stream(x, yq, w) - E(text, p=[p[0] - h]).host_stream(x, yq, w)) / (2 * h)
    assert np.abs(fd - got).max() < 1e-8 * max(1.0, np.abs(got).max())


def test_the_sum_over_the_rule_is_acc_plus_w_times_d():
    rng = np.random.default_rng(13)
    x, yq, w = rng.uniform(0.0, 1.0, (3, 3)), rng.uniform(0.0, 1.0, (6, 3, 2)), np.array([0.2, 0.5, 0.3])
    A = E("exp(p[0]*y[0]) + p[1]", p=[0.7, 0.1])
    got = A.host_tangents(x, yq, w)
    acc = np.zeros((3, 6))
    for q in range(3):
        acc = acc + w[q] * A.host_tangents(x, yq[:, q:q + 1], np.ones(1))[:, 0]
    assert np.array_equal(got[:, 0], acc)
    assert np.array_equal(got[:, 1], np.full((3, 6), ((0.0 + 0.2 * 1.0) + 0.5 * 1.0) + 0.3 * 1.0))


# -- 4. the zero-tangent rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,want", [
    ("sqrt(y[0] - y[0]) + p[0]", [1.0, 0.0]),  # d sqrt(0) would be 0 / 0
    ("p[0] + 1/(y[0] - y[0])*0", [1.0, 0.0]),  # the quotient rule would divide by zero
    ("p[0]*y[1] + log(y[0] - y[0])*p[1]", None),  # p[1] is live through log(0) = -inf: its tangent is -inf, p[0]'s stays finite
    ("where(y[0] < 2, p[0], sqrt(y[0] - 1)*p[1])", [1.0, 0.0]),  # the branch not taken holds NaN
])
def test_a_part_without_the_parameter_cannot_poison_its_tangent(text, want):
    yq = np.array([[[0.25, 0.5]], [[0.75, 0.125]]])
    got = E(text, p=[0.5, 2.0]).host_tangents(np.zeros((1, 3)), yq, np.ones(1))[0]
    if want is None:
        assert np.array_equal(got[0], yq[None, :, 0, 1][0]) and np.all(np.isneginf(got[1]))
    else:
        assert np.array_equal(got, np.array(want)[:, None] * np.ones((2, 2))) and not np.signbit(got).any()


# -- 5. the ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_program_struct_carries_n_params():
    A = E("1 + p[0]*y[0] + p[1]", p=[0.5, 2.0])
    stream = CoefStream.program(np.zeros((2, 1, 2)), np.ones(1), *A.program(), A.n_comp, np.zeros((3, 3)), n_params=A.n_params)
    prog = stream.shared[2]
    assert isinstance(prog, Program) and prog.n_params == 2 and prog.struct().n_params == 2
    assert stream.coef_source().program.contents.n_params == 2
    assert Program(prog.ops, prog.consts, 1).struct().n_params == 0  # the default: a program without parameters
    assert CoefStream.program(np.zeros((2, 1, 2)), np.ones(1), *A.program(), A.n_comp, np.zeros((3, 3))).shared[2].n_params == 0
    assert _lib.CoefProgram.n_params.offset == 12 and C.sizeof(_lib.CoefProgram) == 32
    assert (_lib.PROGRAM_MAX_PARAMS, _lib.DIRS_PARAMETERS) == (expr.MAX_PARAMS, 2)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hommx_hip.h")).read()
    assert "#define HOMMX_PROGRAM_MAX_PARAMS 4" in hdr and "#define HOMMX_DIRS_PARAMETERS 2" in hdr


CONST0 = [(expr.OP_CONST, 0), (expr.OP_STORE, 0)]
SOLVE_ENTRIES = {"hommx_solve_batch_source": (None, PTR, None), "hommx_expand_source_device": (PTR, None),
                 "hommx_expand_tangents": (PTR, PTR), "hommx_expand_tangents_device": (PTR, PTR, None)}


@pytest.mark.parametrize("entry", list(SOLVE_ENTRIES))
@pytest.mark.parametrize("kw,text", [
    (dict(ops=GOOD, prog_n_params=5), "n_params must be 0 .. 4, got 5"),
    (dict(ops=GOOD, prog_n_params=-1), "n_params must be 0 .. 4, got -1"),
    (dict(ops=CONST0, consts=[1.0], prog_n_params=2), "n_params is 2, above n_consts (1)"),
])
def test_n_params_is_validated_on_every_path(lib, entry, kw, text):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    rc, msg = call(lib, entry, C.addressof(fake), 1, source(**kw), SOLVE_ENTRIES[entry])
    assert rc == -1 and text in msg, (rc, msg)


@pytest.mark.parametrize("entry", ["hommx_expand_tangents", "hommx_expand_tangents_device"])
def test_expand_tangents_checks(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan, tail = C.addressof(fake), (None,) if entry.endswith("_device") else ()
    with_p = dict(ops=CONST0, consts=[1.0], prog_n_params=1)
    rc, msg = call(lib, entry, plan, 1, source(ops=GOOD), (PTR, PTR) + tail)
    assert rc == -1 and "the program has no parameters (n_params == 0)" in msg, (rc, msg)
    rc, msg = call(lib, entry, plan, 1, C.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=PTR)), (PTR, PTR) + tail)
    assert rc == -1 and "need a HOMMX_COEF_PROGRAM source, got form 0" in msg, (rc, msg)
    rc, msg = call(lib, entry, plan, 1, source(**with_p), (PTR, None) + tail)
    assert rc == -1 and msg == "null dirs_out", (rc, msg)
    rc, msg = call(lib, entry, plan, 1, source(ops=[(28, 0)], consts=[1.0], prog_n_params=1), (PTR, PTR) + tail)
    assert rc == -1 and "unknown opcode 28" in msg  # the validation of hommx_expand_source comes first
    assert call(lib, entry, None, 0, source(**with_p), (PTR, PTR) + tail)[0] == -1  # a null plan
    assert call(lib, entry, plan, 0, None, (None, None) + tail)[0] == 0  # an empty batch reads nothing
    if tail:
        rc, msg = call(lib, entry, plan, 2**31, source(**with_p), (None, PTR) + tail)
        assert rc == -1 and "too large for one launch" in msg, (rc, msg)


def _sens_call(lib, entry, plan, src, args):
    tail = (None,) if entry.endswith("_device") else ()
    rc = getattr(lib, entry)(plan, 1, src, None, C.byref(args), *tail)
    return rc, lib.hommx_last_error().decode()


@pytest.mark.parametrize("entry", ["hommx_sensitivity_source", "hommx_sensitivity_source_device", "hommx_second_sensitivity_source",
                                   "hommx_second_sensitivity_source_device"])
def test_parameter_directions_checks(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan = C.addressof(fake)
    second = "second" in entry
    par = _lib.DIRS_PARAMETERS

    def args(n_dirs, dirs):
        return _lib.Sens2Args(n_dirs, par, dirs, PTR, None) if second else _lib.SensArgs(n_dirs, par, dirs, PTR, None, None, None, None)

    with_p = dict(ops=[(expr.OP_CONST, 0), (expr.OP_CONST, 1), (expr.OP_ADD, 0), (expr.OP_STORE, 0)], consts=[1.0, 2.0], prog_n_params=2)
    rc, msg = _sens_call(lib, entry, plan, C.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=PTR)), args(2, None))
    assert rc == -1 and "HOMMX_DIRS_PARAMETERS needs a HOMMX_COEF_PROGRAM source, got form 0" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(ops=GOOD), args(1, None))
    assert rc == -1 and "the program has no parameters (n_params == 0)" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(**with_p), args(1, None))
    assert rc == -1 and "n_dirs must be the program's n_params (2), got 1" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(**with_p), args(2, PTR))
    assert rc == -1 and "dirs must be NULL" in msg, (rc, msg)
