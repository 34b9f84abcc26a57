"""Expression coefficients on an MI355X (-m gpu): the stream the bytecode kernel expands against ``Expression.host_stream`` (bitwise for
exactly rounded operations, to the accuracy of the device's math functions otherwise), the program form through the generic solve
entries and the five derived families against the sampled form on that stream (bitwise), against ``TwoPhase``, a failing cell, and
``PoissonHMM`` end to end.  7 cells per shape, so that cells x elements is no multiple of the 256 threads of a block, and 300 cells
of the smallest plan."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child of test_derived_families_do_not_depend_on_chunking
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from hommx_amd import MicroCellPlan, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu
E = hmm.Expression

# name -> (dim, n or None on the jittered 9 x 7 mesh, kind, cells)
SHAPES = {
    "fused5": (2, 5, "poisson", 7),
    "fused17": (2, 17, "poisson", 7),
    "elasticity4": (2, 4, "elasticity", 7),
    "matrix4": (2, 4, "poisson_matrix", 7),
    "poisson3d": (3, 3, "poisson", 7),
    "mesh": (2, None, "poisson", 7),
    "fused3x300": (2, 3, "poisson", 300),
}

# scalar expressions of exactly rounded operations only, positive on the unit cell for x in [0, 1]^3: degrees 0, 2 and 3
EXACT = {
    2: ["where(abs(y[0] - 0.5) < 0.25 or y[1] >= 0.875, 5 + 2*x[0], 1)",
        "1 + x[1] + y[0]*y[1] + min(y[0], 0.5)*max(y[1], x[0])",
        "(2 + y[0] - y[1])**3/(4 + x[2]) + where(y[0] >= 0.5 and not y[1] < 0.25, 1, -x[1]/8)"],
    3: ["where(abs(y[0] - 0.5) < 0.25 or y[2] >= 0.875, 5 + 2*x[0], 1)",
        "1 + x[1] + y[0]*y[2] + min(y[0], 0.5)*max(y[1], x[0])",
        "(2 + y[0] - y[1])**3/(4 + x[2]) + where(y[2] >= 0.5 and not y[1] < 0.25, 1, -x[1]/8)"],
}
DEGREES = [0, 2, 3]


def _expression(kind, dim, k):
    """The k-th exact expression in the shape of the plan kind (the scalar one, a Lame pair or a positive definite matrix built on it)."""
    s = EXACT[dim][k]
    if kind == "poisson":
        return E(s)
    if kind == "elasticity":
        return E(lam=s, mu=f"0.5*({s}) + 1")
    return E([[f"1 + {s}", "0.25*x[1]"], ["0.25*x[1]", f"2 + ({s})/2"]])


@functools.lru_cache(maxsize=None)
def _micro(name):
    dim, n, _, _ = SHAPES[name]
    if n is None:
        return W.jittered_unit_square(9, 7, seed=3)
    return Mm.create_unit_square(n, n) if dim == 2 else Mm.create_unit_cube(n, n, n)


@functools.lru_cache(maxsize=None)
def _plan(name):
    dim, n, kind, _ = SHAPES[name]
    p = MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(_micro(name), kind, load_solve=True)
    assert p.kernel == {"fused5": "fused2d", "fused17": "fused2d", "fused3x300": "fused2d", "mesh": "mesh_front"}.get(name, p.kernel)
    return p


def _midpoints(nc, seed=5):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (nc, 3))


def _points(name, degree):
    bary, w = hmm.micro_quadrature(SHAPES[name][0], degree)
    return np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, _micro(name).cell_vertices())), np.ascontiguousarray(w)


def _stream(name, A, nc=None, x=None):
    """(CoefStream of the program form, the stream the host forms) of expression A on the shape."""
    x = _midpoints(nc or SHAPES[name][3]) if x is None else x
    yq, w = _points(name, A.degree)
    return CoefStream.program(yq, w, *A.program(), A.n_comp, x), A.host_stream(x, yq, w)


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """The k-th exact expression on the shape: (CoefStream, host stream), formed once and shared."""
    dim, _, kind, _ = SHAPES[name]
    A = _expression(kind, dim, k)
    assert A.degree == DEGREES[k]
    return _stream(name, A)


def _M(name, seed=9):
    dim, nc = SHAPES[name][0], SHAPES[name][3]
    rng = np.random.default_rng(seed)
    return np.eye(dim)[None] + 0.2 * rng.uniform(-1.0, 1.0, (nc, dim, dim))


# -- 1. the stream, exactly rounded operations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("name", list(SHAPES))
def test_stream_of_exact_operations_is_the_hosts_bitwise(name, k):
    import torch

    p = _plan(name)
    stream, host = _case(name, k)
    assert host.shape[:2] == (SHAPES[name][3], p.n_el) and (host.shape[0] * p.n_el) % 256 != 0
    assert np.all(host[..., 0] > 0) if host.ndim == 3 else np.all(host > 0)
    assert np.array_equal(p.expand(stream), host)
    # the device entry, into an array that shows a write past the end
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    out = torch.full((host.size + 64,), -7.0, dtype=torch.float64, device=dev)
    p.expand_device(len(stream), stream.coef_source(upload), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    assert np.array_equal(got[:host.size].reshape(host.shape), host) and np.all(got[host.size:] == -7.0)


# -- 2. the stream, math functions ------------------------------------------------------------------------------------------------------
# name -> (c0, c1, the argument, built from exactly rounded operations: both sides see the same bits).  HIP's table of the maximum ULP
# error of its double-precision functions is not among the documents this was developed with, so U_f is measured: the largest distance
# in ULPs between the device's f and NumPy's over the arguments of this very test (every shape below, every quadrature point, pointwise:
# a one-point rule of weight 1 leaves v itself), 2 x that, at least 2 (DESIGN.md section 3 records the run).
FUNCTIONS = {
    "sqrt": (0.25, 1.0, "1 + y[0]*y[1] + x[0]"),
    "sin": (0.25, -2.0, "2*pi*y[0] + x[0]"),
    "cos": (0.25, 0.5, "2*pi*y[1] - x[1]"),
    "tan": (0.25, 1.0, "0.5*y[0] + 0.25*x[0]"),
    "exp": (0.25, 0.5, "y[0] - x[0]"),
    "log": (0.25, 2.0, "1 + y[1] + x[2]"),
    "tanh": (0.25, 1.0, "2*y[0] - x[0]"),
}
MEASURED_ULP = {"sqrt": 0, "sin": 1, "cos": 1, "tan": 1, "exp": 1, "log": 1, "tanh": 1}
FUNCTION_SHAPES = ["fused5", "poisson3d", "mesh"]
NUMPY = {"sqrt": np.sqrt, "sin": np.sin, "cos": np.cos, "tan": np.tan, "exp": np.exp, "log": np.log, "tanh": np.tanh}


def pointwise_ulp(name, f):
    """Largest distance in ULPs between the device's f and NumPy's over the arguments the test of `f` on shape `name` uses."""
    p = _plan(name)
    A = E(f"{f}({FUNCTIONS[f][2]})")
    x = _midpoints(SHAPES[name][3])
    yq, _ = _points(name, E(f"1 + {f}({FUNCTIONS[f][2]})").degree)
    worst = 0.0
    for q in range(yq.shape[1]):
        one = np.ascontiguousarray(yq[:, q:q + 1])
        got = p.expand(CoefStream.program(one, np.ones(1), *A.program(), 1, x))
        want = A.host_stream(x, one, np.ones(1))
        worst = max(worst, float(np.max(np.abs(got - want) / np.spacing(np.abs(want)))))
    return worst


@pytest.mark.parametrize("f", list(FUNCTIONS))
@pytest.mark.parametrize("name", FUNCTION_SHAPES)
def test_stream_of_a_math_function_is_within_its_ulps(name, f):
    c0, c1, arg = FUNCTIONS[f]
    A = E(f"{c0} + {c1}*{f}({arg})")
    stream, host = _stream(name, A)
    x, (yq, _) = stream.per_cell, _points(name, A.degree)
    fmax = np.abs(NUMPY[f](E(arg).components(x.T[:, :, None, None], np.moveaxis(yq, -1, 0)[:, None])[0])).max()
    U = max(2, 2 * MEASURED_ULP[f])
    tol = abs(c1) * (U + 1) * 2.0**-52 * fmax
    err = np.abs(_plan(name).expand(stream) - host).max()
    print(f"{name} {f}: max |device - host| = {err:.3e}, tolerance {tol:.3e} (U_f = {U}, max |f| = {fmax:.4f})")
    assert err <= tol


# -- 3. the solve entries -----------------------------------------------------------------------------------------------------------------
def _solve_device(p, nc, source, M, keep_alive):
    """A_eff and info of a device solve entry given the uploaded source."""
    import torch

    dev = torch.device("cuda", p.device)
    A = torch.full((nc, p.t, p.t), np.nan, dtype=torch.float64, device=dev)
    info = torch.full((nc,), -7, dtype=torch.int32, device=dev)
    Mp = None
    if M is not None:
        keep_alive.append(torch.from_numpy(np.ascontiguousarray(M)).to(dev))
        Mp = keep_alive[-1].data_ptr()
    p.solve_source_device(nc, source, Mp, A.data_ptr(), info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return A.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_solve_entries_equal_the_sampled_stream_bitwise(name, with_M):
    import torch

    p = _plan(name)
    stream, host = _case(name, 2)
    nc = len(stream)
    M = _M(name) if with_M else None
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    want, want_info = _solve_device(p, nc, CoefStream.sampled(host).coef_source(upload), M, keep)  # the sampled form: hommx_solve_batch_device's path
    ref = torch.full((nc, p.t, p.t), np.nan, dtype=torch.float64, device=dev)
    ref_info = torch.full((nc,), -7, dtype=torch.int32, device=dev)
    p.solve_device(nc, upload(host), upload(M) if with_M else None, ref.data_ptr(), ref_info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(ref.cpu().numpy(), want) and np.array_equal(ref_info.cpu().numpy(), want_info)
    assert not want_info.any() and np.all(np.isfinite(want))
    got, info = _solve_device(p, nc, stream.coef_source(upload), M, keep)  # hommx_solve_batch_source_device
    assert np.array_equal(got, want) and np.array_equal(info, want_info)
    got, info = stream.solve(p, M, return_info=True)  # hommx_solve_batch_source
    assert np.array_equal(got, want) and np.array_equal(info, want_info)
    keep2 = []
    stream.solve_device(p, lambda a: (keep2.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev)), keep2[-1].data_ptr())[1],
                        upload(M) if with_M else None, ref.data_ptr(), ref_info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)  # the device twin CoefStream.solve_device names: solve_program_device
    assert np.array_equal(ref.cpu().numpy(), want) and np.array_equal(ref_info.cpu().numpy(), want_info)


# -- 4. the derived families -------------------------------------------------------------------------------------------------------------
def _derived(p, coef, M, seed=21):
    """Every derived family's output for the coefficient (a CoefStream or a sampled array), as one dict of arrays."""
    nc = len(coef)
    rng = np.random.default_rng(seed)
    xi = rng.standard_normal((nc, p.t))
    dirs = rng.uniform(0.5, 1.5, (2, p.n_el))
    P = rng.standard_normal((1, p.n_el, p.t))
    r = p.reconstruct(coef, xi, M, fields=True)
    s = p.sensitivities(coef, M, directions=dirs)
    lo = p.loads(coef, P, M)
    st = p.stratification_sensitivities(coef, M)
    s2 = p.second_sensitivities(coef, M, directions=dirs, first=True)
    out = {"stats": np.concatenate([r.mean_strain, r.mean_flux, r.energy[:, None], r.max_flux[:, None], r.argmax_element[:, None]], axis=1),
           "strain": r.strain, "flux": r.flux, "dA": s.dA, "P_eff": lo.P_eff, "dA_dM": st.dA_dM, "d2A": s2.d2A, "dA2": s2.dA}
    for k, res in enumerate((r, s, lo, st, s2)):
        out[f"A{k}"], out[f"info{k}"] = res.A_eff, res.info
    return out


@pytest.mark.parametrize("name", ["fused5", "mesh"])
def test_derived_families_equal_the_sampled_form_bitwise(name):
    p = _plan(name)
    stream, host = _case(name, 2)
    M = _M(name)
    got, want = _derived(p, stream, M), _derived(p, host, M)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
        assert np.all(np.isfinite(want[key])), key
    assert not want["info0"].any()


CHUNK_CELLS = 60  # a fused n = 5 cell holds 43 KB of factor record, refinement scratch and correctors: 1 MB takes 24 of them


def _chunk_case():
    x = _midpoints(CHUNK_CELLS, seed=31)
    stream, host = _stream("fused5", _expression("poisson", 2, 2), x=x)
    M = np.eye(2)[None] + 0.2 * np.random.default_rng(33).uniform(-1.0, 1.0, (CHUNK_CELLS, 2, 2))
    return _derived(_plan("fused5"), stream, M), host, M


def test_derived_families_do_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the program form in chunks of 1 MB."""
    here, host, M = _chunk_case()
    want = _derived(_plan("fused5"), host, M)
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, HOMMX_RECON_MEM_MB="1"), timeout=300)
    child = np.load(out)
    for key in want:
        assert np.array_equal(here[key], want[key]) and np.array_equal(child[key], want[key]), key


# -- 5. against TwoPhase -------------------------------------------------------------------------------------------------------------------
def test_where_equals_two_phase_bitwise():
    msh, micro = Mm.create_unit_square(3, 3), Mm.create_unit_square(8, 8)
    tp = hmm.TwoPhase(lambda y: np.abs(y[0] - 0.5) < 0.25, lambda x: 5 + 2 * x[0], lambda x: 1.0 + 0.0 * x[0])
    a = hmm.PoissonHMM(msh, tp, lambda x: 1.0, micro, 0.01)
    b = hmm.PoissonHMM(msh, E("where(abs(y[0] - 0.5) < 0.25, 5 + 2*x[0], 1)"), lambda x: 1.0, micro, 0.01)
    cells = np.arange(msh.num_cells)
    assert b._coef_stream(cells)[0].method == "solve_program" and b.quadrature_degree_used == 0
    (Aa, ia), (Ab, ib) = a._effective_tensors(cells), b._effective_tensors(cells)
    assert np.array_equal(Aa, Ab) and np.array_equal(ia, ib) and not ia.any()
    assert np.abs(Aa[:, 0, 0] - Aa[:, 1, 1]).min() > 0.1  # a laminate: the two directions differ


# -- 6. a bad cell -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused5", "poisson3d", "mesh"])
def test_bad_cell_is_flagged_alone(name):
    p = _plan(name)
    A = E("1.5 - x[0] + 0.25*y[0]*y[1]")  # negative throughout a cell whose x[0] is 3
    x = _midpoints(7, seed=13)
    good, _ = _stream(name, A, x=x)
    x_bad = x.copy()
    x_bad[4, 0] = 3.0
    bad, host = _stream(name, A, x=x_bad)
    assert np.all(host[4] < 0) and np.all(np.delete(host, 4, axis=0) > 0)
    M = _M(name)
    (Ag, ig), (Ab, ib) = good.solve(p, M, return_info=True), bad.solve(p, M, return_info=True)
    assert not ig.any() and ib[4] != 0 and not np.delete(ib, 4).any()
    keep = [0, 1, 2, 3, 5, 6]
    assert np.array_equal(Ab[keep], Ag[keep])


# -- 7. end to end -------------------------------------------------------------------------------------------------------------------------
def test_poisson_hmm_end_to_end(caplog):
    msh, micro = Mm.create_unit_square(8, 8), Mm.create_unit_square(8, 8)
    f = lambda x: 1.0 + x[0]
    h = hmm.PoissonHMM(msh, E("1.1 + x[0] + sin(2*pi*y[0])"), f, micro, 0.01)
    g = hmm.PoissonHMM(msh, lambda x, y: 1.1 + x[0] + np.sin(2 * np.pi * y[0]), f, micro, 0.01, quadrature_degree=3)
    u, v = h.solve().x.array.copy(), g.solve().x.array.copy()
    assert h.quadrature_degree_used == 3 and not [r for r in caplog.records if r.levelname == "WARNING"]
    assert not h.cell_info.any() and not g.cell_info.any()
    err = np.abs(u - v).max() / np.abs(v).max()
    print(f"device-sampled expression against the host-sampled callable: max rel. difference of u {err:.2e}")
    assert err < 1e-10 and np.abs(v).max() > 1e-3


if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case()[0])
