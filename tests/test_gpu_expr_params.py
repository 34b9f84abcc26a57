"""Parameters of expression coefficients on an MI355X (-m gpu): the forward-mode passes of the interpreter k_expand_program<P> against
``Expression.host_tangents`` (bitwise for exactly rounded operations, to the accuracy of the device's math functions otherwise), the
derivative families with ``directions="parameters"`` against the same calls on the sampled stream and sampled tangents (bitwise, host
and device entries, any chunking), against ``TwoPhase``, a failing cell, and the solver classes end to end against central differences
taken with ``set_parameters``.  The shapes are those of test_gpu_expr.py: 7 cells each, so that cells x elements is no multiple of the
128 or 64 threads of a block, and 300 cells of the smallest plan."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child of test_parameter_directions_do_not_depend_on_chunking
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import test_gpu_expr as G
from hommx_amd import hmm, mesh as Mm
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu
E = hmm.Expression
SHAPES, FUNCTION_SHAPES, MEASURED_ULP = G.SHAPES, G.FUNCTION_SHAPES, G.MEASURED_ULP

# scalar expressions of exactly rounded operations only, positive on the unit cell for x in [0, 1]^3, with 1, 2, 3 and 4 parameters
# ({z}: the last fast variable of the shape); 3 parameters run the kernel of 4 with a dead tangent
EXACT = [
    ("1 + x[1] + p[0]*y[0]*{z} + min(y[0], 0.5)*max({z}, x[0])", [0.75]),
    ("where(abs(y[0] - 0.5) < 0.25 or {z} >= 0.875, p[0] + 2*x[0], p[1])", [5.0, 1.0]),
    ("p[0] + p[1]*y[0]*(1 - y[0]) + p[2]*x[0]*{z}", [1.5, 2.0, 0.5]),
    ("(p[0] + y[0] - y[1])**3/(4 + x[2]) + where({z} >= 0.5 and not y[1] < 0.25, p[1], -x[1]/8) + abs(p[2]*(y[0] - 0.5)) + max(p[3]*{z}, 0.25)",
     [2.0, 1.0, -0.5, 0.75]),
]


def _expression(kind, dim, k):
    """The k-th exact expression in the shape of the plan kind (the scalar one, a Lame pair or a positive definite matrix built on it)."""
    text, p = EXACT[k]
    s = text.format(z="y[1]" if dim == 2 else "y[2]")
    if kind == "poisson":
        return E(s, p=p)
    if kind == "elasticity":
        return E(lam=s, mu=f"0.5*({s}) + 1", p=p)
    return E([[f"1 + {s}", "0.25*x[1]*p[0]"], ["0.25*x[1]*p[0]", f"2 + ({s})/2"]], p=p)


def _stream(name, A, nc=None, x=None):
    """(CoefStream of the program form with its parameters, the points and weights of the rule, the midpoints)."""
    x = G._midpoints(nc or SHAPES[name][3]) if x is None else x
    yq, w = G._points(name, A.degree)
    return CoefStream.program(yq, w, *A.program(), A.n_comp, x, n_params=A.n_params), yq, w, x


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """The k-th exact expression on the shape: (CoefStream, host stream, host tangents), formed once and shared."""
    dim, _, kind, _ = SHAPES[name]
    A = _expression(kind, dim, k)
    stream, yq, w, x = _stream(name, A)
    return stream, A.host_stream(x, yq, w), A.host_tangents(x, yq, w)


def _uploader(dev, keep):
    import torch

    def upload(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    return upload


# -- 1. the tangents, exactly rounded operations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(EXACT)))
@pytest.mark.parametrize("name", list(SHAPES))
def test_tangents_of_exact_operations_are_the_hosts_bitwise(name, k):
    import torch

    p = G._plan(name)
    stream, host, tangents = _case(name, k)
    nc, n_params = SHAPES[name][3], len(EXACT[k][1])
    assert tangents.shape[:3] == (nc, n_params, p.n_el) and (nc * p.n_el) % 64 != 0
    assert np.all(np.isfinite(tangents)) and all(np.abs(tangents[:, j]).max() > 0 for j in range(n_params))
    coef, dirs = p.expand_tangents(stream)
    assert np.array_equal(dirs, tangents)
    assert np.array_equal(coef, p.expand(stream)) and np.array_equal(coef, host)
    # the device entry, into arrays that show a write past the end; then the tangents alone
    dev = torch.device("cuda", p.device)
    keep = []
    src = stream.coef_source(_uploader(dev, keep))
    st = torch.cuda.current_stream(dev).cuda_stream
    for with_coef in (True, False):
        out_c = torch.full((host.size + 64,), -7.0, dtype=torch.float64, device=dev)
        out_d = torch.full((tangents.size + 64,), -7.0, dtype=torch.float64, device=dev)
        p.expand_tangents_device(nc, src, out_c.data_ptr() if with_coef else None, out_d.data_ptr(), st)
        torch.cuda.synchronize(dev)
        got_c, got_d = out_c.cpu().numpy(), out_d.cpu().numpy()
        assert np.array_equal(got_d[:tangents.size].reshape(tangents.shape), tangents) and np.all(got_d[tangents.size:] == -7.0)
        if with_coef:
            assert np.array_equal(got_c[:host.size].reshape(host.shape), host) and np.all(got_c[host.size:] == -7.0)
        else:
            assert np.all(got_c == -7.0)


# -- 2. the tangents, math functions -----------------------------------------------------------------------------------------------------
# A = c0 + c1 f(p[0] * arg) at p[0] = 1 with the arguments of test_gpu_expr.py (p[0] * arg = arg exactly, and its tangent is
# add(mul(p[0], 0), mul(1, arg)) = arg exactly), so host and device apply the rule of f to the same bits a = arg, da = arg and differ by
# the device's math functions and the roundings behind them.  With u = 2^-52 (one ulp, relative) and U_g = max(2, 2 MEASURED_ULP[g])
# ulps for the device function g the rule calls, counting one ulp per rounded arithmetic operation of the rule (host and device round
# different inputs), the rule's result t differs by at most K u D, D the largest magnitude of the rule's term over the points:
#   sqrt  t = da / (2 v), v = sqrt(a)      K = U_sqrt + 1   (2 v is exact, the quotient rounds)         D = max |da / (2 v)|
#   sin   t = cos(a) da                    K = U_cos + 1                                                 D = max |cos(a) da|
#   cos   t = -(sin(a) da)                 K = U_sin + 1                                                 D = max |sin(a) da|
#   tan   t = da (1 + v v), v = tan(a)     K = 2 U_tan + 3  (v v: 2 U + 1; the sum and the product)      D = max |da (1 + v v)|
#   exp   t = v da, v = exp(a)             K = U_exp + 1                                                 D = max |v da|
#   log   t = da / a                       K = 1            (no device function)                         D = max |da / a|
#   tanh  t = da (1 - v v), v = tanh(a)    K = 2 U_tanh + 3 (absolute, against 1 >= v v: no relative bound survives the cancellation)
#                                                                                                          D = max |da|
# Behind the rule: the product with c1 (1), the product with the weight (1), and n_q additions of the sum, on terms whose weights sum
# to W = sum |w_q| in magnitude:  |device - host| <= |c1| (K + 2 + n_q) u W D.
RULES = {
    "sqrt": ("sqrt", lambda U: U + 1, lambda a: a / (2 * np.sqrt(a))),
    "sin": ("cos", lambda U: U + 1, lambda a: np.cos(a) * a),
    "cos": ("sin", lambda U: U + 1, lambda a: np.sin(a) * a),
    "tan": ("tan", lambda U: 2 * U + 3, lambda a: a * (1 + np.tan(a) ** 2)),
    "exp": ("exp", lambda U: U + 1, lambda a: np.exp(a) * a),
    "log": (None, lambda U: 1, lambda a: a / a),
    "tanh": ("tanh", lambda U: 2 * U + 3, lambda a: a),
}


@pytest.mark.parametrize("f", list(G.FUNCTIONS))
@pytest.mark.parametrize("name", FUNCTION_SHAPES)
def test_tangents_of_a_math_function_are_within_its_ulps(name, f):
    c0, c1, arg = G.FUNCTIONS[f]
    A = E(f"{c0} + {c1}*{f}(p[0]*({arg}))", p=[1.0])
    stream, yq, w, x = _stream(name, A)
    a = E(arg).components(x.T[:, :, None, None], np.moveaxis(yq, -1, 0)[:, None])[0]
    g, K, term = RULES[f]
    U = 0 if g is None else max(2, 2 * MEASURED_ULP[g])
    D = np.abs(term(a)).max()
    tol = abs(c1) * (K(U) + 2 + len(w)) * 2.0**-52 * np.abs(w).sum() * D
    coef, dirs = G._plan(name).expand_tangents(stream)
    host = A.host_tangents(x, yq, w)
    err = np.abs(dirs - host).max()
    print(f"{name} {f}: max |device - host| of the tangent = {err:.3e}, tolerance {tol:.3e} (U = {U}, K = {K(U)}, n_q = {len(w)}, D = {D:.4f})")
    assert np.all(np.isfinite(host)) and np.abs(host).max() > 0.05
    assert err <= tol
    assert np.array_equal(coef, G._plan(name).expand(stream))  # the value part is the value pass's (k_expand_program<0>), whatever the functions


# -- 3. the derivative families ----------------------------------------------------------------------------------------------------------
def _families(p, coef, M, **dirs):
    s = p.sensitivities(coef, M, **dirs)
    s2 = p.second_sensitivities(coef, M, first=True, **dirs)
    return {"dA": s.dA, "A": s.A_eff, "info": s.info, "d2A": s2.d2A, "dA2": s2.dA, "A2": s2.A_eff, "info2": s2.info}


def _families_device(p, stream, M, n_params):
    """The same through the device entries with per_cell="parameters"."""
    import torch

    dev = torch.device("cuda", p.device)
    keep = []
    upload = _uploader(dev, keep)
    nc, t = len(stream), p.t
    st = torch.cuda.current_stream(dev).cuda_stream
    new = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device=dev)
    dA, A, d2A, dA2, A2 = new(nc, n_params, t, t), new(nc, t, t), new(nc, n_params, n_params, t, t), new(nc, n_params, t, t), new(nc, t, t)
    info, info2 = (torch.full((nc,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    src = stream.coef_source(upload)
    Mp = None if M is None else upload(M)
    p.sensitivities_device(nc, src, Mp, n_params, None, "parameters", dA.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(), stream=st)
    p.second_sensitivities_device(nc, src, Mp, n_params, None, d2A.data_ptr(), "parameters", dA2.data_ptr(), A2.data_ptr(), info2.data_ptr(), st)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in dict(dA=dA, A=A, info=info, d2A=d2A, dA2=dA2, A2=A2, info2=info2).items()}


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_parameter_directions_equal_sampled_directions_bitwise(name, with_M):
    p = G._plan(name)
    k = 3 if SHAPES[name][3] < 100 else 1  # four parameters; two on the 300 cells
    stream, host, tangents = _case(name, k)
    M = G._M(name) if with_M else None
    want = _families(p, host, M, directions=tangents, per_cell=True)
    assert not want["info"].any() and not want["info2"].any()
    assert all(np.all(np.isfinite(v)) for v in want.values()) and np.abs(want["d2A"]).max() > 0
    got = _families(p, stream, M, directions="parameters")
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    got = _families_device(p, stream, M, tangents.shape[1])
    for key in want:
        assert np.array_equal(got[key], want[key]), ("device", key)


def test_parameter_directions_need_a_program_with_parameters():
    p = G._plan("fused5")
    stream, host, _ = _case("fused5", 0)
    plain = G._case("fused5", 0)[0]  # a program without parameters
    for coef in (host, plain, CoefStream.sampled(host)):
        with pytest.raises(ValueError, match='directions="parameters" needs'):
            p.sensitivities(coef, directions="parameters")
        with pytest.raises(ValueError, match='directions="parameters" needs'):
            p.second_sensitivities(coef, directions="parameters")
    with pytest.raises(ValueError, match='directions="parameters" needs'):
        p.expand_tangents(plain)


# -- 4. chunking -------------------------------------------------------------------------------------------------------------------------
CHUNK_CELLS = 60  # a fused n = 5 cell holds 43 KB of factor record, refinement scratch and correctors: 1 MB takes some 20 of them


def _chunk_case():
    x = G._midpoints(CHUNK_CELLS, seed=31)
    stream, yq, w, _ = _stream("fused5", _expression("poisson", 2, 3), x=x)
    M = np.eye(2)[None] + 0.2 * np.random.default_rng(33).uniform(-1.0, 1.0, (CHUNK_CELLS, 2, 2))
    return _families(G._plan("fused5"), stream, M, directions="parameters")


def test_parameter_directions_do_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the same calls in chunks of 1 MB."""
    here = _chunk_case()
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, HOMMX_RECON_MEM_MB="1"), timeout=300)
    child = np.load(out)
    for key in here:
        assert np.array_equal(child[key], here[key]), key
    assert not here["info"].any() and np.all(np.isfinite(here["d2A"]))


# -- 5. against TwoPhase -----------------------------------------------------------------------------------------------------------------
def test_where_on_two_parameters_equals_two_phase_bitwise(caplog):
    msh, micro = Mm.create_unit_square(3, 3), Mm.create_unit_square(8, 8)
    tp = hmm.TwoPhase(lambda y: np.abs(y[0] - 0.5) < 0.25, lambda x: 5.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
    a = hmm.PoissonHMM(msh, tp, lambda x: 1.0, micro, 0.01)
    b = hmm.PoissonHMM(msh, E("where(abs(y[0] - 0.5) < 0.25, p[1], p[0])", p=[1.0, 5.0], parameter_names=("outside", "inside")),
                       lambda x: 1.0, micro, 0.01)
    assert b.quadrature_degree_used == 0 and not [r for r in caplog.records if r.levelname == "WARNING"]  # no parameter in the comparison
    ra, rb = a.tensor_derivatives(), b.tensor_derivatives()
    assert ra.names == rb.names == ("outside", "inside")
    assert np.array_equal(ra.dA, rb.dA) and np.array_equal(ra.A_eff, rb.A_eff) and np.array_equal(ra.info, rb.info) and not ra.info.any()
    assert np.abs(ra.dA[:, 0]).max() > 0.1 and np.abs(ra.dA[:, 1]).max() > 0.01  # both phases carry a derivative


# -- 6. a bad cell -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused5", "poisson3d", "mesh"])
def test_bad_cell_is_flagged_alone(name):
    p = G._plan(name)
    A = E("p[0] - x[0] + p[1]*y[0]*y[1]", p=[1.5, 0.25])  # negative throughout a cell whose x[0] is 3
    x = G._midpoints(7, seed=13)
    x_bad = x.copy()
    x_bad[4, 0] = 3.0
    (good, yq, w, _), (bad, _, _, _) = _stream(name, A, x=x), _stream(name, A, x=x_bad)
    host = A.host_stream(x_bad, yq, w)
    assert np.all(host[4] < 0) and np.all(np.delete(host, 4, axis=0) > 0)
    M = G._M(name)
    g, b = _families(p, good, M, directions="parameters"), _families(p, bad, M, directions="parameters")
    keep = [0, 1, 2, 3, 5, 6]
    for key in ("info", "info2"):
        assert not g[key].any() and b[key][4] != 0 and not b[key][keep].any()
    for key in g:
        assert np.array_equal(b[key][keep], g[key][keep]), key


# -- 7. end to end -----------------------------------------------------------------------------------------------------------------------
def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


STEP = 1e-5  # step and tolerance of test_gpu_sensitivity.py::test_poisson_hmm_end_to_end: the same kernel against the same kind of difference


def test_poisson_hmm_end_to_end(caplog):
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(8, 8)
    p0 = np.array([0.5, 2.0])
    h = hmm.PoissonHMM(msh, E("1.1 + x[0] + p[0]*sin(2*pi*y[0]) + p[1]*y[1]*(1-y[1])", p=p0), lambda x: 1.0 + x[0], micro, 0.01)
    assert h._coeff.affine_in_parameters
    u = h.solve().x.array.copy()
    plan = h._plan
    r = h.tensor_derivatives()
    assert r.names == ("p0", "p1") and r.dA.shape == (msh.num_cells, 2, 2, 2) and not r.info.any()
    _close(r.A_eff, h.effective_tensors, 1e-12, "A_eff of the corrector route against the tensor route")
    e = h.energy_derivatives()
    s2 = h.tensor_second_derivatives()
    assert s2.names == ("p0", "p1") and s2.d2A.shape == (msh.num_cells, 2, 2, 2, 2) and np.array_equal(s2.dA, r.dA)
    assert e.shape == (msh.num_cells, 2) and h.energy_second_derivatives().shape == (msh.num_cells, 2, 2)
    assert not [rec for rec in caplog.records if rec.levelname == "WARNING"]
    fd2 = np.empty_like(s2.d2A)
    for k in range(2):
        side = []
        for sign in (+1.0, -1.0):
            q = p0.copy()
            q[k] += sign * STEP
            h.set_parameters(q)
            assert h._needs_reassembly and h._plan is plan and h._coeff.p.tolist() == q.tolist()
            h.solve()  # reassembles: the tensors and the macro matrix at q
            assert not h._needs_reassembly and h._plan is plan and not h.cell_info.any()
            side.append((h.effective_tensors.copy(), h._A.copy(), h.tensor_derivatives().dA))
        (Ap, Kp, dp), (Am, Km, dm) = side
        assert np.abs(Ap - Am).max() > 0
        _close(r.dA[:, k], (Ap - Am) / (2 * STEP), 1e-6, f"d A_H / d p{k} against central differences")
        fd_e = (u @ (Kp @ u) - u @ (Km @ u)) / (2 * STEP)
        err = abs(e[:, k].sum() - fd_e) / abs(fd_e)
        print(f"d (u . K_H u) / d p{k} against central differences", err)
        assert err < 1e-6
        fd2[:, :, k] = (dp - dm) / (2 * STEP)
    _close(s2.d2A, fd2, 1e-6, "d2 A_H / dp dp against central differences of dA")
    h.set_parameters(p0)
    assert np.array_equal(h.tensor_derivatives(cells=[3, 20]).dA, r.dA[[3, 20]])
    for bad in ([0.5], [0.5, 2.0, 1.0]):
        with pytest.raises(ValueError):
            h.set_parameters(bad)
    with pytest.raises(ValueError, match="set_parameters"):
        hmm.PoissonHMM(msh, E("1.1 + x[0]"), lambda x: 1.0, micro, 0.01).set_parameters([1.0])
    with pytest.raises(ValueError, match="no parameters"):  # an Expression without parameters keeps its error
        hmm.PoissonHMM(msh, E("1.1 + x[0] + y[0]"), lambda x: 1.0, micro, 0.01).tensor_derivatives()


def test_second_derivatives_need_an_expression_affine_in_its_parameters():
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(8, 8)
    h = hmm.PoissonHMM(msh, E("1.5 + tanh(p[0]*(y[0]-0.5))", p=[3.0], parameter_names=("steepness",)), lambda x: 1.0, micro, 0.01)
    with pytest.raises(ValueError, match="not affine in its parameters") as err:
        h.tensor_second_derivatives()
    assert "directions=[" in str(err.value)
    r = h.tensor_derivatives()
    assert r.names == ("steepness",) and not r.info.any()
    side = []
    for sign in (+1.0, -1.0):
        h.set_parameters([3.0 + sign * STEP])
        h._assemble_stiffness()
        side.append(h.effective_tensors.copy())
    _close(r.dA[:, 0], (side[0] - side[1]) / (2 * STEP), 1e-6, "d A_H / d steepness against central differences")


# -- 8. elasticity -----------------------------------------------------------------------------------------------------------------------
def test_linear_elasticity_hmm():
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(4, 4)
    h = hmm.LinearElasticityHMM(msh, E(lam="1.25", mu="5 + p[0]*sin(2*pi*y[0])", p=[4.5]), lambda x: np.zeros(2), micro, 0.01)
    r = h.tensor_derivatives()
    assert r.names == ("p0",) and r.dA.shape == (msh.num_cells, 1, 3, 3) and r.A_eff.shape == (msh.num_cells, 3, 3) and not r.info.any()
    s2 = h.tensor_second_derivatives()
    assert s2.d2A.shape == (msh.num_cells, 1, 1, 3, 3) and np.array_equal(s2.dA, r.dA)
    side = []
    for sign in (+1.0, -1.0):
        h.set_parameters([4.5 + sign * STEP])
        h._assemble_stiffness()
        assert not h.cell_info.any()
        side.append(h.effective_tensors.copy())
    _close(r.dA[:, 0], (side[0] - side[1]) / (2 * STEP), 1e-6, "d C_H / d p0 against central differences")


if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case())
