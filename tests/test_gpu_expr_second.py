"""Second-order forward mode of expression coefficients on an MI355X (-m gpu): the passes of k_expand_program2<P> against
``Expression.host_second_tangents`` (bitwise for exactly rounded operations, to the accuracy of the device's math functions otherwise),
their value and tangent streams against ``expand_tangents`` (bitwise), the smallest and the largest stack, the Hessian of
``second_sensitivities(directions="parameters", curvature=True)`` against the same calls on sampled streams (bitwise, host and device
entries, any chunking), and the solver classes end to end against central differences of ``tensor_derivatives``.  The shapes are those
of test_gpu_expr.py: 7 cells each, so that cells x elements is no multiple of the 64 threads of a block, and 300 cells of the smallest
plan."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child of test_the_hessian_does_not_depend_on_chunking
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import test_gpu_expr as G
import test_gpu_expr_params as P1
from hommx_amd import expr, hmm, mesh as Mm
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu
E = hmm.Expression
SHAPES, FUNCTION_SHAPES, MEASURED_ULP = G.SHAPES, G.FUNCTION_SHAPES, G.MEASURED_ULP

# Scalar expressions of exactly rounded operations only, positive on the unit cell for x in [0, 1]^3 (and fields in [0, 1]): (text,
# p, n_fields, the pairs whose stream is not zero).  The four of test_gpu_expr_params.py with 1, 2, 3 and 4 parameters -- three of them
# affine, the last cubic in p[0] --; the same with the square of the sum of all parameters, so that every pair has curvature (3
# and 4 slots run one launch per pair of slots); and two parameters with two fields, products and powers among them
_ALL = lambda n: tuple((a, b) for a in range(n) for b in range(a, n))
_SQUARE = lambda n: "(" + " + ".join(f"p[{j}]" for j in range(n)) + ")**2*y[0]"  # short: the Lame pair of the last one has 112 of 128 instructions
CASES = [(text, p, 0, ((0, 0),) if k == 3 else ()) for k, (text, p) in enumerate(P1.EXACT)]
CASES += [(f"{text} + {_SQUARE(len(p))}", p, 0, _ALL(len(p))) for text, p in P1.EXACT]
CASES += [("1 + x[1] + p[0]*f[0]*y[0] + (p[0] + 2*p[1] + f[0] + 3*f[1])**2*{z}/4 + p[1]**2*f[1]*y[0] + f[0]**3*min(y[0], 0.5)", [0.75, 1.5], 2,
           _ALL(4))]
HESSIAN_CASES = [5, 7]  # two and four parameters, every pair with curvature
AFFINE_CASE = 1


def _expression(kind, dim, k):
    """The k-th case in the shape of the plan kind (the scalar one, a Lame pair or a positive definite matrix built on it)."""
    text, p, n_fields, _ = CASES[k]
    s = text.format(z="y[1]" if dim == 2 else "y[2]")
    kw = dict(p=p, fields=n_fields) if n_fields else dict(p=p)
    if kind == "poisson":
        return E(s, **kw)
    if kind == "elasticity":
        return E(lam=s, mu=f"0.5*({s}) + 1", **kw)
    return E([[f"1 + {s}", "0.25*x[1]*p[0]"], ["0.25*x[1]*p[0]", f"2 + ({s})/2"]], **kw)


def _rows(nc, n_fields, seed=5):
    """The midpoints of test_gpu_expr.py, then n_fields fields in [0, 1]."""
    x = G._midpoints(nc, seed)
    return np.hstack([x, np.random.default_rng(seed + 100).uniform(0.0, 1.0, (nc, n_fields))]) if n_fields else x


def _stream(name, A, nc=None, x=None):
    """(CoefStream of the program form with its parameters and fields, the points and weights of the rule, the rows)."""
    x = _rows(nc or SHAPES[name][3], A.n_fields) if x is None else x
    yq, w = G._points(name, A.degree)
    return CoefStream.program(yq, w, *A.program(), A.n_comp, x, n_params=A.n_params, n_fields=A.n_fields), yq, w, x


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """The k-th case on the shape: (CoefStream, host stream, host tangents, host second-order streams), formed once and shared."""
    dim, _, kind, _ = SHAPES[name]
    A = _expression(kind, dim, k)
    stream, yq, w, x = _stream(name, A)
    return stream, A.host_stream(x, yq, w), A.host_tangents(x, yq, w), A.host_second_tangents(x, yq, w)


def _pair(a, b, n):
    a, b = min(a, b), max(a, b)
    return a * n - a * (a - 1) // 2 + (b - a)


def _device_expand(p, stream, shapes, with_first):
    """hommx_expand_second_tangents_device into arrays with a guard tail: (coef, dirs, curv) as NumPy arrays (None: not asked for)."""
    import torch

    dev = torch.device("cuda", p.device)
    keep = []
    src = stream.coef_source(P1._uploader(dev, keep))
    st = torch.cuda.current_stream(dev).cuda_stream
    outs = [torch.full((int(np.prod(s)) + 64,), -7.0, dtype=torch.float64, device=dev) for s in shapes]
    p.expand_second_tangents_device(len(stream), src, outs[0].data_ptr() if with_first else None, outs[1].data_ptr() if with_first else None,
                                    outs[2].data_ptr(), st)
    torch.cuda.synchronize(dev)
    got = []
    for k, (o, s) in enumerate(zip(outs, shapes)):
        a, n = o.cpu().numpy(), int(np.prod(s))
        assert np.all(a[n:] == -7.0), "a write past the end"
        if k < 2 and not with_first:
            assert np.all(a == -7.0)
            got.append(None)
        else:
            got.append(a[:n].reshape(s))
    return got


# -- 1. exactly rounded operations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)))
@pytest.mark.parametrize("name", list(SHAPES))
def test_second_tangents_of_exact_operations_are_the_hosts_bitwise(name, k):
    p = G._plan(name)
    stream, host, tangents, second = _case(name, k)
    nc, n_tan, live = SHAPES[name][3], len(CASES[k][1]) + CASES[k][2], CASES[k][3]
    pairs = _ALL(n_tan)
    assert second.shape[:3] == (nc, len(pairs), p.n_el) and (nc * p.n_el) % 64 != 0 and np.all(np.isfinite(second))
    for s, ab in enumerate(pairs):
        assert (np.abs(second[:, s]).max() > 0) == (ab in live), ab
    coef, dirs, curv = p.expand_second_tangents(stream)
    assert np.array_equal(curv, second)
    first = p.expand_tangents(stream)
    assert np.array_equal(coef, first[0]) and np.array_equal(dirs, first[1])
    assert np.array_equal(coef, host) and np.array_equal(dirs, tangents)
    for s, ab in enumerate(pairs):
        assert (np.abs(curv[:, s]).max() > 0) == (ab in live), ab
    # the device entry, into arrays that show a write past the end; then the second-order streams alone
    shapes = (host.shape, tangents.shape, second.shape)
    got = _device_expand(p, stream, shapes, True)
    assert np.array_equal(got[0], host) and np.array_equal(got[1], tangents) and np.array_equal(got[2], second)
    got = _device_expand(p, stream, shapes, False)
    assert np.array_equal(got[2], second)


# -- 2. the smallest and the largest stack -----------------------------------------------------------------------------------------------
def _deep(levels):
    """p[0]*(y[0] + p[1]*(y[1] + p[0]*( ... ))): every level holds two more entries."""
    text = "1"
    for k in reversed(range(levels)):
        text = f"p[{k % 2}]*(y[{k % 2}]/4 + {text})"
    return "1 + " + text


@pytest.mark.parametrize("name", ["fused5", "poisson3d", "mesh", "fused3x300"])
def test_stack_of_one_row_and_of_sixteen(name):
    p = G._plan(name)
    deep = E(_deep(7), p=[0.75, 0.5])
    shallow = E("p[0]", p=[1.5])
    assert max(expr.stack_depths(deep.program()[0].tolist())) == expr.MAX_STACK == 16
    assert max(expr.stack_depths(shallow.program()[0].tolist())) == 1  # p[0]**2 is DUP MUL: two rows
    for A in (deep, shallow):
        stream, yq, w, x = _stream(name, A)
        coef, dirs, curv = p.expand_second_tangents(stream)
        assert np.array_equal(curv, A.host_second_tangents(x, yq, w))
        assert np.array_equal(dirs, A.host_tangents(x, yq, w)) and np.array_equal(coef, A.host_stream(x, yq, w))
        assert (np.abs(curv).max() > 0) == (A is deep)


# -- 3. math functions -------------------------------------------------------------------------------------------------------------------
# A = c0 + c1 f(p[0] * arg) at p[0] = 1 with the arguments of test_gpu_expr.py, as in test_gpu_expr_params.py section 2: the operand of f
# is a = arg, da = arg exactly on both sides, and ha = add(add(add(mul(1, 0), mul(0, arg)), mul(1, 0)), mul(0, 1)) = 0 exactly, so in
# every rule the term with ha is an exact zero and its sum with the other term is exact.  Host and device differ by the device's math
# functions and the roundings behind them.  u = 2^-52, U_g = max(2, 2 MEASURED_ULP[g]) ulps for the device function g, one ulp per
# rounded operation (host and device round different inputs).  d is the rule's own first-order tangent, whose error
# test_gpu_expr_params.py derives (K_1 below); the second-order result t differs by at most K u D:
#   sqrt  t = -((2 d) d) / (2 v), d = da / (2 v)      d: K_1 = U + 1; (2 d) d: 2 K_1 + 1; 2 v: U; the quotient: 1
#                                                      K = 3 U + 4                               D = max |da^2 / (4 v^3)|
#   sin   t = -((v da) da), v = sin(a)                 v: U; two products                         K = U + 2,  D = max |sin(a) da^2|
#   cos   t = -((v da) da), v = cos(a)                 likewise                                   K = U + 2,  D = max |cos(a) da^2|
#   tan   t = ((2 v) d) da, d = da (1 + v v)           d: K_1 = 2 U + 3; 2 v: U; two products     K = 3 U + 5
#                                                                                                 D = max |2 v da^2 (1 + v v)|
#   tanh  t = -(((2 v) d) da), d = da (1 - v v)        d: (2 U + 3) u |da| ABSOLUTE (cancellation against 1), and |d| <= |da|; 2 v: U;
#                                                      two products                               K = 3 U + 5,  D = max |2 v da^2|
#   exp   t = d da, d = v da                           d: K_1 = U + 1; one product                K = U + 2,  D = max |v da^2|
#   log   t = -(da d) / a, d = da / a                  d: 1; the product 1; the quotient 1        K = 3,      D = max |da^2 / a^2| = 1
# Behind the rule: the product with c1 (the MUL rule's other three terms are exact zeros), the product with the weight, and n_q
# additions of the sum on terms whose weights sum to W = sum |w_q|:  |device - host| <= |c1| (K + 2 + n_q) u W D.
RULES2 = {
    "sqrt": ("sqrt", lambda U: 3 * U + 4, lambda a: a * a / (4 * np.sqrt(a) ** 3)),
    "sin": ("sin", lambda U: U + 2, lambda a: np.sin(a) * a * a),
    "cos": ("cos", lambda U: U + 2, lambda a: np.cos(a) * a * a),
    "tan": ("tan", lambda U: 3 * U + 5, lambda a: 2 * np.tan(a) * a * a * (1 + np.tan(a) ** 2)),
    "exp": ("exp", lambda U: U + 2, lambda a: np.exp(a) * a * a),
    "log": (None, lambda U: 3, lambda a: a / a),
    "tanh": ("tanh", lambda U: 3 * U + 5, lambda a: 2 * np.tanh(a) * a * a),
}


@pytest.mark.parametrize("f", list(G.FUNCTIONS))
@pytest.mark.parametrize("name", FUNCTION_SHAPES)
def test_second_tangents_of_a_math_function_are_within_its_ulps(name, f):
    c0, c1, arg = G.FUNCTIONS[f]
    A = E(f"{c0} + {c1}*{f}(p[0]*({arg}))", p=[1.0])
    stream, yq, w, x = _stream(name, A)
    a = E(arg).components(x.T[:, :, None, None], np.moveaxis(yq, -1, 0)[:, None])[0]
    g, K, term = RULES2[f]
    U = 0 if g is None else max(2, 2 * MEASURED_ULP[g])
    D = np.abs(term(a)).max()
    tol = abs(c1) * (K(U) + 2 + len(w)) * 2.0**-52 * np.abs(w).sum() * D
    plan = G._plan(name)
    coef, dirs, curv = plan.expand_second_tangents(stream)
    host = A.host_second_tangents(x, yq, w)
    err = np.abs(curv - host).max()
    print(f"{name} {f}: max |device - host| of the second-order stream = {err:.3e}, tolerance {tol:.3e} (U = {U}, K = {K(U)}, "
          f"n_q = {len(w)}, D = {D:.4f})")
    assert np.all(np.isfinite(host)) and np.abs(host).max() > 0.01
    assert err <= tol
    first = plan.expand_tangents(stream)  # value and tangents are the first-order pass's, whatever the functions
    assert np.array_equal(coef, first[0]) and np.array_equal(dirs, first[1])


# -- 4. the Hessian at the plan level ----------------------------------------------------------------------------------------------------
def _hessian(p, stream, M):
    r = p.second_sensitivities(stream, M, directions="parameters", curvature=True, first=True)
    return {"d2A": r.d2A, "dA": r.dA, "A": r.A_eff, "info": r.info}


def _hessian_device(p, stream, M, n_tan):
    import torch

    dev = torch.device("cuda", p.device)
    keep = []
    upload = P1._uploader(dev, keep)
    nc, t = len(stream), p.t
    st = torch.cuda.current_stream(dev).cuda_stream
    new = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device=dev)
    d2A, dA, A = new(nc, n_tan, n_tan, t, t), new(nc, n_tan, t, t), new(nc, t, t)
    info = torch.full((nc,), -7, dtype=torch.int32, device=dev)
    p.second_sensitivities_device(nc, stream.coef_source(upload), None if M is None else upload(M), n_tan, None, d2A.data_ptr(), "parameters",
                                  dA.data_ptr(), A.data_ptr(), info.data_ptr(), st, curvature=True)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in dict(d2A=d2A, dA=dA, A=A, info=info).items()}


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("k", HESSIAN_CASES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_hessian_is_the_tangent_block_plus_the_curvature_term_bitwise(name, k, with_M):
    p = G._plan(name)
    stream, host, tangents, second = _case(name, k)
    n_tan, n_pairs = tangents.shape[1], second.shape[1]
    M = G._M(name) if with_M else None
    along = p.second_sensitivities(host, M, directions=tangents, per_cell=True)
    dAk = np.concatenate([p.sensitivities(host, M, directions=second[:, s:s + 8], per_cell=True).dA for s in range(0, n_pairs, 8)], axis=1)
    assert dAk.shape[1] == n_pairs and np.all(np.isfinite(dAk)) and all(np.abs(dAk[:, s]).max() > 0 for s in range(n_pairs))
    want = np.empty_like(along.d2A)
    for a in range(n_tan):
        for b in range(n_tan):
            want[:, a, b] = along.d2A[:, a, b] + dAk[:, _pair(a, b, n_tan)]  # one float64 addition
    plain = p.second_sensitivities(stream, M, directions="parameters", first=True)
    assert np.array_equal(plain.d2A, along.d2A) and not plain.info.any()
    for got in (_hessian(p, stream, M), _hessian_device(p, stream, M, n_tan)):
        assert np.array_equal(got["d2A"], want) and np.abs(want - along.d2A).max() > 0
        assert np.array_equal(got["dA"], plain.dA) and np.array_equal(got["A"], plain.A_eff) and np.array_equal(got["info"], plain.info)
        assert np.array_equal(got["d2A"], got["d2A"].transpose(0, 2, 1, 3, 4)) and np.array_equal(got["d2A"], got["d2A"].transpose(0, 1, 2, 4, 3))


@pytest.mark.parametrize("name", ["fused5", "elasticity4", "mesh"])
def test_hessian_of_an_affine_expression_is_the_default_calls(name):
    p = G._plan(name)
    stream = _case(name, AFFINE_CASE)[0]
    M = G._M(name)
    plain = p.second_sensitivities(stream, M, directions="parameters", first=True)
    got = _hessian(p, stream, M)
    assert np.all(got["d2A"] == plain.d2A) and np.abs(plain.d2A).max() > 0
    assert np.array_equal(got["dA"], plain.dA) and np.array_equal(got["A"], plain.A_eff) and not got["info"].any()


def test_curvature_is_for_parameter_directions_only():
    p = G._plan("fused5")
    stream, host, tangents, _ = _case("fused5", 5)
    with pytest.raises(ValueError, match='curvature=True needs directions="parameters"'):
        p.second_sensitivities(host, directions=tangents, per_cell=True, curvature=True)
    with pytest.raises(ValueError, match='directions="parameters" needs'):
        p.second_sensitivities(host, directions="parameters", curvature=True)
    with pytest.raises(ValueError, match='directions="parameters" needs'):
        p.expand_second_tangents(G._case("fused5", 0)[0])  # a program without parameters


# -- 5. chunking -------------------------------------------------------------------------------------------------------------------------
CHUNK_CELLS = 60  # as in test_gpu_expr_params.py: 1 MB takes some 20 fused n = 5 cells, fewer with the ten second-order streams


def _chunk_case():
    x = G._midpoints(CHUNK_CELLS, seed=31)
    stream, yq, w, _ = _stream("fused5", _expression("poisson", 2, 7), x=x)
    M = np.eye(2)[None] + 0.2 * np.random.default_rng(33).uniform(-1.0, 1.0, (CHUNK_CELLS, 2, 2))
    return _hessian(G._plan("fused5"), stream, M)


def test_the_hessian_does_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the same call in chunks of 1 MB."""
    here = _chunk_case()
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, HOMMX_RECON_MEM_MB="1"), timeout=300)
    child = np.load(out)
    for key in here:
        assert np.array_equal(child[key], here[key]), key
    assert not here["info"].any() and np.all(np.isfinite(here["d2A"]))


# -- 6. end to end -----------------------------------------------------------------------------------------------------------------------
STEP, TOL = 1e-5, 1e-6  # step and tolerance of test_gpu_expr_params.py::test_poisson_hmm_end_to_end: the same kind of difference


def _error(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def test_poisson_hmm_hessian_end_to_end():
    """kappa_11 = 0.5 y[1] >= 0 with mean 0.25: dA_H[kappa_11] is positive definite and of order 0.1 against A_H of order 1."""
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(8, 8)
    p0 = np.array([3.0, 1.2])
    h = hmm.PoissonHMM(msh, E("1.5 + tanh(p[0]*(y[0]-0.3)) + 0.25*p[1]**2*y[1]", p=p0), lambda x: 1.0 + x[0], micro, 0.01)
    assert not h._coeff.affine_in_parameters
    h.solve()
    with pytest.raises(ValueError, match="not affine in its parameters") as err:
        h.tensor_second_derivatives()
    assert "directions=[" in str(err.value) and "curvature=True" in str(err.value)
    s2 = h.tensor_second_derivatives(curvature=True)
    r = h.tensor_derivatives()
    assert s2.names == ("p0", "p1") and s2.d2A.shape == (msh.num_cells, 2, 2, 2, 2) and np.array_equal(s2.dA, r.dA) and not s2.info.any()
    assert h.energy_second_derivatives(curvature=True).shape == (msh.num_cells, 2, 2)
    cells = h._local_cells()
    stream, kind = h._coef_stream(cells)
    along = h._ensure_plan(kind).second_sensitivities(stream, h._stratification(cells), directions="parameters").d2A
    fd2 = np.empty_like(s2.d2A)
    for k in range(2):
        side = []
        for sign in (+1.0, -1.0):
            q = p0.copy()
            q[k] += sign * STEP
            h.set_parameters(q)
            side.append(h.tensor_derivatives().dA)
        fd2[:, :, k] = (side[0] - side[1]) / (2 * STEP)
    h.set_parameters(p0)
    err, err_along = _error(s2.d2A, fd2), _error(along, fd2)
    print(f"d2 A_H / dp dp against central differences of dA: {err:.3e} with the curvature term, {err_along:.3e} along the tangents alone")
    assert err < TOL
    assert err_along > 100 * TOL  # the curvature term cannot hide inside the tolerance
    assert np.linalg.eigvalsh(s2.d2A[:, 1, 1] - along[:, 1, 1]).min() > 0.01  # dA_H[kappa_11]: positive definite, of order 0.1


INCLUSION_N = 4  # the micro mesh of the smooth inclusion (see the test)


def test_poisson_hmm_hessian_in_a_field_end_to_end():
    """The README's smooth inclusion, one radius per macro cell.  INCLUSION_N: the smallest micro mesh of 4, 8, 12, 16, 24, 32 cells
    across on which the first-derivative check of test_gpu_expr_fields.py (dA against central differences of A_H, STEP, TOL) passes
    for this expression.  It passes on all six (7.3e-8, 3.8e-8, 1.9e-8, 4.2e-8, 2.7e-8, 7.1e-9: both sides are exact on the discrete
    problem, whatever it resolves), so n = 4, the smallest micro mesh of the solver-class tests; the second-derivative check measured
    7.5e-8 there and 2.0e-7 .. 2.7e-7 on the finer ones."""
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(INCLUSION_N, INCLUSION_N)
    A = E("1 + 9/(1 + exp(((y[0]-0.5)**2 + (y[1]-0.5)**2 - f[0]**2)*200))", fields=("radius",))
    h = hmm.PoissonHMM(msh, A, lambda x: 1.0, micro, 0.01)
    f0 = 0.15 + 0.2 * msh.cell_midpoints()[:, 0]
    h.set_fields(f0)
    s2 = h.tensor_second_derivatives(curvature=True)
    assert s2.names == ("radius",) and s2.d2A.shape == (msh.num_cells, 1, 1, 2, 2) and not s2.info.any()
    side = []
    for sign in (+1.0, -1.0):  # every cell reads its own radius alone: one difference serves all cells
        h.set_fields(f0 + sign * STEP)
        h._assemble_stiffness()
        assert not h.cell_info.any()
        side.append((h.effective_tensors.copy(), h.tensor_derivatives().dA))
    h.set_fields(f0)
    e1 = _error(s2.dA[:, 0], (side[0][0] - side[1][0]) / (2 * STEP))
    e2 = _error(s2.d2A[:, 0, 0], (side[0][1][:, 0] - side[1][1][:, 0]) / (2 * STEP))
    print(f"smooth inclusion, n = {INCLUSION_N}: dA against differences of A_H {e1:.3e}, d2A against differences of dA {e2:.3e}")
    assert e1 < TOL and e2 < TOL


def test_linear_elasticity_hmm_hessian():
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(4, 4)
    h = hmm.LinearElasticityHMM(msh, E(lam="1.25", mu="5 + p[0]*sin(2*pi*y[0])*p[0]", p=[2.0]), lambda x: np.zeros(2), micro, 0.01)
    assert not h._coeff.affine_in_parameters
    s2 = h.tensor_second_derivatives(curvature=True)
    assert s2.names == ("p0",) and s2.d2A.shape == (msh.num_cells, 1, 1, 3, 3) and not s2.info.any()
    side = []
    for sign in (+1.0, -1.0):
        h.set_parameters([2.0 + sign * STEP])
        side.append(h.tensor_derivatives().dA)
    h.set_parameters([2.0])
    err = _error(s2.d2A[:, 0, 0], (side[0][:, 0] - side[1][:, 0]) / (2 * STEP))
    print(f"d2 C_H / dp0 dp0 against central differences of dC_H: {err:.3e}")
    assert err < TOL


def test_curvature_needs_a_device_sampled_expression_with_slots():
    msh, micro = Mm.create_unit_square(3, 3), Mm.create_unit_square(4, 4)
    tp = hmm.TwoPhase(lambda y: np.abs(y[0] - 0.5) < 0.25, lambda x: 5.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
    with pytest.raises(ValueError, match="curvature=True needs a device-sampled Expression.*TwoPhase"):
        hmm.PoissonHMM(msh, tp, lambda x: 1.0, micro, 0.01).tensor_second_derivatives(curvature=True)
    h = hmm.PoissonHMM(msh, E("1.5 + p[0]**2*y[0]", p=[1.0]), lambda x: 1.0, micro, 0.01)
    with pytest.raises(ValueError, match="curvature=True needs a device-sampled Expression.*directions="):
        h.tensor_second_derivatives(directions=[lambda x, y: 1.0 + 0.0 * y[0]], curvature=True)
    with pytest.raises(ValueError, match="neither parameters"):
        hmm.PoissonHMM(msh, E("1.5 + y[0]"), lambda x: 1.0, micro, 0.01).tensor_second_derivatives(curvature=True)


if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case())
