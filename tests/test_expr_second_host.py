"""Second-order forward mode of an ``Expression`` on the CPU: ``host_second_tangents`` (include/hommx_hip.h,
hommx_expand_second_tangents; the NumPy twin of k_expand_program2) in closed form on dyadic data, every rule of ``_TANGENT2`` against
central differences of ``host_tangents``, the dead rule, and the validation of hommx_expand_second_tangents and of
HOMMX_DIRS_PARAMETERS_CURVATURE at the C ABI, which runs on the host before the plan's device is made current (the manner of
test_expr_params_host.py).  No GPU needed."""

import ctypes as C
import os

import numpy as np
import pytest

from hommx_amd import _lib, expr
from hommx_amd.expr import Expression as E
from test_program_abi_host import GOOD, P as PTR, call, source
from test_reconstruct_source_host import _fake_plan

# two elements of two quadrature points each, dyadic coordinates and weights: every sum below is exact
YQ = np.array([[[0.25, 0.5], [0.75, 0.125]], [[0.5, 0.25], [0.125, 0.875]]])
W = np.array([0.25, 0.5])
X = np.array([[0.5, 0.25, 0.125], [0.75, 0.5, 0.25]])
YSUM = np.einsum("q,eq->e", W, YQ[:, :, 0])  # sum_q w_q y[0] of every element


# -- 1. closed forms, bitwise ------------------------------------------------------------------------------------------------------------
def test_pairs_are_the_abis_row_major_order():
    assert E("p[0]", p=[1.0]).pairs == ((0, 0),)
    assert E("p[0] + p[1]", p=[1.0, 2.0]).pairs == ((0, 0), (0, 1), (1, 1))
    assert E("p[0] + f[0]*f[1]", p=[1.0], fields=2).pairs == ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    assert len(E("p[0]", p=[1.0, 2.0, 3.0, 4.0]).pairs) == 10 and E("p[0]", p=[1.0, 2.0, 3.0, 4.0]).pairs[4] == (1, 1)
    with pytest.raises(ValueError, match="no parameters"):
        E("y[0]").host_second_tangents(X, YQ, W)


def test_a_square_and_a_product_in_closed_form():
    h = E("p[0]**2*y[0]", p=[3.0]).host_second_tangents(X, YQ, W)
    assert h.shape == (2, 1, 2) and np.array_equal(h[:, 0], np.broadcast_to(2 * YSUM, (2, 2)))
    A = E("p[0]*p[1]*y[0]", p=[3.0, 5.0])
    h = A.host_second_tangents(X, YQ, W)
    assert h.shape == (2, 3, 2) and A.pairs[1] == (0, 1)
    assert np.array_equal(h[:, 1], np.broadcast_to(YSUM, (2, 2)))
    assert np.array_equal(h[:, 0], np.zeros((2, 2))) and np.array_equal(h[:, 2], np.zeros((2, 2))) and not np.signbit(h).any()
    # the mixed pair is symmetric under renaming the parameters
    B = E("p[1]*p[0]*y[0]", p=[5.0, 3.0])
    assert np.array_equal(B.host_second_tangents(X, YQ, W)[:, 1], h[:, 1])
    C2 = E("(p[0] + 2*p[1])**2*y[0]", p=[3.0, 5.0]).host_second_tangents(X, YQ, W)
    D2 = E("(p[1] + 2*p[0])**2*y[0]", p=[5.0, 3.0]).host_second_tangents(X, YQ, W)
    assert np.array_equal(C2[:, 1], D2[:, 1]) and np.array_equal(C2[:, 0], D2[:, 2]) and np.array_equal(C2[:, 2], D2[:, 0])
    assert np.array_equal(C2[:, 0], np.broadcast_to(2 * YSUM, (2, 2))) and np.array_equal(C2[:, 2], np.broadcast_to(8 * YSUM, (2, 2)))


def test_an_affine_expression_has_no_curvature():
    A = E("1 + x[0] + p[0]*sin(2*pi*y[0]) + p[1]*y[1]*(1 - y[1]) + f[0]/(2 + y[0])", p=[0.5, 2.0], fields=1)
    assert A.affine_in_parameters
    h = A.host_second_tangents(np.hstack([X, [[0.3], [0.6]]]), YQ, W)
    assert h.shape == (2, 6, 2) and np.array_equal(h, np.zeros_like(h)) and not np.signbit(h).any()


def test_the_value_and_the_tangents_are_those_of_the_first_order_pass():
    A = E(lam="1 + p[0]**2*y[0]/(1 + p[1])", mu="2 + tanh(p[0]*y[1])*p[1]", p=[0.5, 2.0])
    v1, d1 = expr._run(A._ops.tolist(), A._consts, 2, X.T[:, :, None], np.moveaxis(YQ[:, 0], -1, 0)[:, None, :], 2, 0)
    v2, d2, h2 = expr._run(A._ops.tolist(), A._consts, 2, X.T[:, :, None], np.moveaxis(YQ[:, 0], -1, 0)[:, None, :], 2, 0, second=True)
    for c in range(2):
        assert np.array_equal(v1[c], v2[c]) and all(np.array_equal(d1[c][j], d2[c][j]) for j in range(2))
    assert A.host_second_tangents(X, YQ, W).shape == (2, 3, 2, 2)


# -- 2. every rule against central differences of the tangents -----------------------------------------------------------------------------
STEP, TOL = 1e-5, 1e-6  # the step and tolerance of tests/test_gpu_expr_params.py for the same kind of difference

RULE_CASES = [
    ("add sub neg", "p[0]**2*y[0] - (-(p[1]*p[0]**2)) + p[1]**3", [1.5, 0.75], 0),
    ("mul", "(p[0]*y[0] + p[1])*(p[0]*p[1] + y[1])*p[1]", [1.5, 0.75], 0),
    ("div", "(p[0] + y[0])/(1 + p[1]*p[0] + p[0]**2*y[1])", [1.5, 0.75], 0),
    ("abs", "abs(p[0]**2*(y[0] - 0.4) - p[1]**2*y[1])", [1.5, 0.75], 0),
    ("min max", "min(p[0]**2*y[0], p[1]**3*y[1]) + max(p[0]*p[1], 1.5*p[0]**2*y[0])", [1.5, 0.75], 0),
    ("where", "where(y[0] < 0.4, p[0]**3*y[1], p[0]*p[1]**2 + y[0])", [1.5, 0.75], 0),  # branches of different curvature
    ("sqrt", "sqrt(1 + p[0]**2*y[0] + p[1]*y[1])", [1.5, 0.75], 0),
    ("sin", "sin(p[0]*y[0] + p[1]**2*y[1])", [1.5, 0.75], 0),
    ("cos", "cos(p[0]*p[1]*y[0] + y[1])", [1.5, 0.75], 0),
    ("tan", "tan(0.3*p[0]*y[0] + 0.2*p[1]**2*y[1])", [1.5, 0.75], 0),
    ("exp", "exp(p[0]*y[0] - p[1]**2*y[1])", [1.5, 0.75], 0),
    ("log", "log(1 + p[0]**2*y[0] + p[1]*p[0]*y[1])", [1.5, 0.75], 0),
    ("tanh", "tanh(p[0]*(y[0] - 0.3)) + 0.25*p[1]**2*y[1]", [3.0, 1.2], 0),
    ("a parameter with a field", "1 + 9/(1 + exp(((y[0]-0.5)**2 + (y[1]-0.5)**2 - f[0]**2)*p[0]))", [20.0], 1),
    ("four slots", "p[0]*p[1]*y[0] + p[2]**2*p[3] + p[3]*p[0]/(1 + p[1]**2)*y[1]", [1.5, 0.75, 2.0, 0.5], 0),
]


@pytest.mark.parametrize("what,text,p,n_fields", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_rule_against_central_differences_of_the_tangents(what, text, p, n_fields):
    A = E(text, p=p, fields=n_fields) if n_fields else E(text, p=p)
    x = np.hstack([X, np.array([[0.3], [0.2]])[:, :n_fields]]) if n_fields else X
    h = A.host_second_tangents(x, YQ, W)
    n_tan, pairs = A.n_params + A.n_fields, A.pairs
    assert h.shape == (2, len(pairs), 2) and np.all(np.isfinite(h))
    fd = np.empty((2, n_tan, n_tan, 2))  # d (tangent a) / d (slot b)
    for b in range(n_tan):
        side = []
        for sign in (+1.0, -1.0):
            q, xs = np.array(p), x.copy()
            if b < A.n_params:
                q[b] += sign * STEP
            else:
                xs[:, 3 + b - A.n_params] += sign * STEP
            side.append(A.with_parameters(q).host_tangents(xs, YQ, W))
        fd[:, :, b] = (side[0] - side[1]) / (2 * STEP)
    for s, (a, b) in enumerate(pairs):
        scale = np.abs(fd).max()
        for other in (fd[:, a, b], fd[:, b, a]):
            err = np.abs(h[:, s] - other).max() / scale
            print(f"{what}: pair {(a, b)}: max |h - difference| / max |difference| = {err:.3e}")
            assert err < TOL, (what, (a, b), err)
    assert np.abs(h).max() > 0.01  # the case has curvature at all


# -- 3. the dead rule --------------------------------------------------------------------------------------------------------------------
def test_a_part_that_does_not_read_both_slots_cannot_poison_the_pair():
    x = np.zeros((1, 3))
    h = E("sqrt(y[0] - y[0]) + p[0]**2", p=[3.0]).host_second_tangents(x, YQ, W)[0]  # d2 sqrt(0) would be 0 / 0
    assert np.array_equal(h[0], np.full(2, 2 * W.sum()))
    h = E("sqrt(y[0] - y[0]) + p[0]**2 + p[1]", p=[3.0, 1.0]).host_second_tangents(x, YQ, W)[0]
    assert np.array_equal(h, np.array([2 * W.sum(), 0.0, 0.0])[:, None] * np.ones((3, 2))) and not np.signbit(h).any()
    # a division by zero in a part that reads only p[1]: its own pair (1, 1) is live and not finite, the pairs with p[0] are dead
    h = E("p[0]**2*y[0] + p[1]/(y[0] - y[0])*0", p=[3.0, 2.0]).host_second_tangents(x, YQ, W)[0]
    assert np.array_equal(h[0], 2 * YSUM) and np.array_equal(h[1], np.zeros(2)) and not np.signbit(h[:2]).any()
    # the same division in a part that reads only p[1], additively: every pair is finite, the dead ones +0.0
    h = E("p[0]**2*y[0] + (p[1] + 1/(y[0] - y[0]))", p=[3.0, 2.0]).host_second_tangents(x, YQ, W)[0]
    assert np.array_equal(h, np.stack([2 * YSUM, np.zeros(2), np.zeros(2)])) and not np.signbit(h).any()
    # the branch not taken holds NaN in its value and in its own curvature
    h = E("where(y[0] < 2, p[0]*p[1], sqrt(y[0] - 1)*p[1]**2) + p[0]**2*y[0]", p=[3.0, 2.0]).host_second_tangents(x, YQ, W)[0]
    assert np.array_equal(h, np.stack([2 * YSUM, np.full(2, W.sum()), np.zeros(2)]))
    h = E("1/(y[0] - y[0])*0 + p[0]**2 + p[1]", p=[3.0, 1.0]).host_second_tangents(x, YQ, W)[0]
    assert np.array_equal(h, np.array([2 * W.sum(), 0.0, 0.0])[:, None] * np.ones((3, 2))) and not np.signbit(h).any()


# -- 4. the ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


CONST0 = [(expr.OP_CONST, 0), (expr.OP_STORE, 0)]


def test_the_header_and_the_bindings_agree():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hommx_hip.h")).read()
    assert "#define HOMMX_DIRS_PARAMETERS_CURVATURE 3" in hdr and _lib.DIRS_PARAMETERS_CURVATURE == 3
    for name in ("hommx_expand_second_tangents", "hommx_expand_second_tangents_device"):
        assert name + "(" in hdr and name in _lib.EXPORTED_SYMBOLS


@pytest.mark.parametrize("entry", ["hommx_expand_second_tangents", "hommx_expand_second_tangents_device"])
def test_expand_second_tangents_checks(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan, tail = C.addressof(fake), (None,) if entry.endswith("_device") else ()
    with_p = dict(ops=CONST0, consts=[1.0], prog_n_params=1)
    rc, msg = call(lib, entry, plan, 1, source(ops=GOOD), (PTR, PTR, PTR) + tail)
    assert rc == -1 and "the program has no parameters (n_params == 0)" in msg, (rc, msg)
    rc, msg = call(lib, entry, plan, 1, C.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=PTR)), (PTR, PTR, PTR) + tail)
    assert rc == -1 and "need a HOMMX_COEF_PROGRAM source, got form 0" in msg, (rc, msg)
    for ptrs in ((PTR, PTR, None), (None, None, None)):
        rc, msg = call(lib, entry, plan, 1, source(**with_p), ptrs + tail)
        assert rc == -1 and msg == "null curv_out", (rc, msg)
    rc, msg = call(lib, entry, plan, 1, source(ops=[(28, 0)], consts=[1.0], prog_n_params=1), (PTR, PTR, PTR) + tail)
    assert rc == -1 and "unknown opcode 28" in msg  # the validation of hommx_expand_source comes first
    assert call(lib, entry, None, 0, source(**with_p), (PTR, PTR, PTR) + tail)[0] == -1  # a null plan
    assert call(lib, entry, plan, 0, None, (None, None, None) + tail)[0] == 0  # an empty batch reads nothing
    if tail:
        rc, msg = call(lib, entry, plan, 2**31, source(**with_p), (None, None, PTR) + tail)
        assert rc == -1 and "too large for one launch" in msg, (rc, msg)


def _sens_call(lib, entry, plan, src, args):
    tail = (None,) if entry.endswith("_device") else ()
    rc = getattr(lib, entry)(plan, 1, src, None, C.byref(args), *tail)
    return rc, lib.hommx_last_error().decode()


WITH_P = dict(ops=[(expr.OP_CONST, 0), (expr.OP_CONST, 1), (expr.OP_MUL, 0), (expr.OP_STORE, 0)], consts=[1.0, 2.0], prog_n_params=2)


@pytest.mark.parametrize("entry", ["hommx_sensitivity_source", "hommx_sensitivity_source_device"])
def test_first_derivatives_refuse_the_curvature_code(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    args = _lib.SensArgs(2, _lib.DIRS_PARAMETERS_CURVATURE, None, PTR, None, None, None, None)
    rc, msg = _sens_call(lib, entry, C.addressof(fake), source(**WITH_P), args)
    assert rc == -1 and "HOMMX_DIRS_PARAMETERS_CURVATURE is a value of per_cell in hommx_sens2_args only" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ["hommx_second_sensitivity_source", "hommx_second_sensitivity_source_device"])
def test_curvature_directions_checks(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan = C.addressof(fake)
    args = lambda n_dirs, dirs, d2A=PTR: _lib.Sens2Args(n_dirs, _lib.DIRS_PARAMETERS_CURVATURE, dirs, d2A, None)
    rc, msg = _sens_call(lib, entry, plan, C.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=PTR)), args(2, None))
    assert rc == -1 and "needs a HOMMX_COEF_PROGRAM source, got form 0" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(ops=GOOD), args(1, None))
    assert rc == -1 and "the program has no parameters (n_params == 0)" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(**WITH_P), args(1, None))
    assert rc == -1 and "n_dirs must be the program's n_params (2), got 1" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(**WITH_P), args(2, PTR))
    assert rc == -1 and "dirs must be NULL" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(**WITH_P), args(2, None, None))
    assert rc == -1 and "null dirs / d2A" in msg, (rc, msg)


# -- 5. the Python layer -----------------------------------------------------------------------------------------------------------------
def test_curvature_needs_parameter_directions():
    from hommx_amd.batch import MicroCellPlan

    plan = object.__new__(MicroCellPlan)  # no device: the check comes before anything of the plan is read
    with pytest.raises(ValueError, match='curvature=True needs directions="parameters"'):
        plan.second_sensitivities(np.ones((1, 50)), directions=np.ones((1, 50)), curvature=True)
    with pytest.raises(ValueError, match='curvature=True needs per_cell="parameters"'):
        plan.second_sensitivities_device(1, None, None, 1, 1, 1, per_cell=True, curvature=True)
