"""Fields ``f[k]`` of expression coefficients on an MI355X (-m gpu): the value pass and the forward-mode pass of the interpreter
(csrc/coef_program.hip) against ``Expression.host_stream`` / ``host_tangents`` (bitwise for exactly rounded operations, to the accuracy
of the device's math functions otherwise), a field with one value in every cell against the parameter it then is, the position of a
cell's row (permutations, chunks), the derived families against the same calls on the sampled stream and sampled tangents, and the
solver classes end to end: central differences in the field of ONE cell, and a solution-dependent coefficient in a Picard loop.  The
shapes are those of test_gpu_expr.py: 7 cells each, so that cells x elements is no multiple of the 64, 128 or 256 threads of a block,
and 300 cells of the smallest plan.  Field values differ from cell to cell in every test but the one that says otherwise, so that a
wrong stride or chunk offset cannot cancel out."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child of test_field_directions_do_not_depend_on_chunking
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import test_gpu_expr as G
from hommx_amd import hmm, mesh as Mm
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu
E = hmm.Expression
SHAPES, FUNCTION_SHAPES, MEASURED_ULP = G.SHAPES, G.FUNCTION_SHAPES, G.MEASURED_ULP


def _rows(nc, n_fields, seed=5, lo=0.5, hi=1.5):
    """Midpoints of test_gpu_expr.py with n_fields values per cell after them, all different."""
    v = np.random.default_rng(seed + 100).uniform(lo, hi, (nc, n_fields))
    return np.ascontiguousarray(np.concatenate([G._midpoints(nc, seed), v], axis=1))


def _stream(name, A, rows=None):
    """(CoefStream of the program form with its parameters and fields, the points and weights of the rule, the rows)."""
    rows = _rows(SHAPES[name][3], A.n_fields) if rows is None else rows
    yq, w = G._points(name, A.degree)
    return CoefStream.program(yq, w, *A.program(), A.n_comp, rows, n_params=A.n_params, n_fields=A.n_fields), yq, w, rows


def _shaped(kind, s, **kw):
    """The scalar text in the shape of the plan kind (the scalar one, a Lame pair or a positive definite matrix built on it)."""
    if kind == "poisson":
        return E(s, **kw)
    if kind == "elasticity":
        return E(lam=s, mu=f"0.5*({s}) + 1", **kw)
    return E([[f"1 + {s}", "0.25*x[1]*f[0]"], ["0.25*x[1]*f[0]", f"2 + ({s})/2"]], **kw)


def _uploader(dev, keep):
    import torch

    def upload(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    return upload


# scalar expressions of exactly rounded operations only, positive on the unit cell for x in [0, 1]^3 and fields in [0.5, 1.5]
# ({z}: the last fast variable of the shape): (text, parameter values, number of fields); 1, 2, 3 and 4 differentiable slots in mixes
# of p and f, and 1, 2 and 4 fields; 3 slots run the kernel of 4 with a dead tangent
EXACT = [
    ("1 + x[1] + f[0]*y[0]*{z} + min(y[0], 0.5)*max({z}, x[0])", None, 1),
    ("where(abs(y[0] - 0.5) < 0.25 or {z} >= 0.875, f[0] + 2*x[0], f[1])", None, 2),
    ("p[0] + f[0]*y[0]*(1 - y[0]) + x[0]*{z}", [1.5], 1),
    ("p[0] + f[1]*y[0]*(1 - y[0]) + f[0]*x[0]*{z}", [1.5], 2),
    ("p[1] + p[0]*y[0]*(1 - y[0]) + f[0]*x[0]*{z}", [2.0, 0.75], 1),
    ("(f[3] + y[0] - y[1])**3/(4 + x[2]) + where({z} >= 0.5 and not y[1] < 0.25, f[1], -x[1]/8) + abs(f[2]*(y[0] - 0.5)) + max(f[0]*{z}, 0.25) + 2",
     None, 4),
    ("(p[0] + y[0] - y[1])**3/(4 + x[2]) + where({z} >= 0.5 and not y[1] < 0.25, f[1], -x[1]/8) + abs(p[1]*(y[0] - 0.5)) + max(f[0]*{z}, 0.25)",
     [2.0, -0.5], 2),
]
FOUR_FIELDS, TWO_AND_TWO, TWO_FIELDS = 5, 6, 1


def _expression(kind, dim, k):
    text, p, n_fields = EXACT[k]
    return _shaped(kind, text.format(z="y[1]" if dim == 2 else "y[2]"), p=p, fields=n_fields)


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """The k-th exact expression on the shape: (CoefStream, host stream, host tangents), formed once and shared."""
    dim, _, kind, _ = SHAPES[name]
    A = _expression(kind, dim, k)
    stream, yq, w, rows = _stream(name, A)
    return stream, A.host_stream(rows, yq, w), A.host_tangents(rows, yq, w)


# -- 1. + 2. the value pass and the tangents, exactly rounded operations -----------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(EXACT)))
@pytest.mark.parametrize("name", list(SHAPES))
def test_stream_and_tangents_of_exact_operations_are_the_hosts_bitwise(name, k):
    import torch

    p = G._plan(name)
    stream, host, tangents = _case(name, k)
    nc, n_tan = SHAPES[name][3], len(EXACT[k][1] or ()) + EXACT[k][2]
    assert stream.per_cell.shape == (nc, 3 + EXACT[k][2]) and len(np.unique(stream.per_cell[:, 3:])) == nc * EXACT[k][2]
    assert tangents.shape[:3] == (nc, n_tan, p.n_el) and (nc * p.n_el) % 64 != 0
    assert np.all(np.isfinite(tangents)) and all(np.abs(tangents[:, j]).max() > 0 for j in range(n_tan)) and host.min() > 0
    assert np.array_equal(p.expand(stream), host)
    coef, dirs = p.expand_tangents(stream)
    assert np.array_equal(coef, host)
    assert np.array_equal(dirs, tangents)
    # the device entries, into arrays that show a write past the end
    dev = torch.device("cuda", p.device)
    keep = []
    src = stream.coef_source(_uploader(dev, keep))
    assert src.n_fields == EXACT[k][2]
    st = torch.cuda.current_stream(dev).cuda_stream
    out_c = torch.full((host.size + 64,), -7.0, dtype=torch.float64, device=dev)
    p.expand_device(nc, src, out_c.data_ptr(), st)
    torch.cuda.synchronize(dev)
    got_c = out_c.cpu().numpy()
    assert np.array_equal(got_c[:host.size].reshape(host.shape), host) and np.all(got_c[host.size:] == -7.0)
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
# The construction and the bound of test_gpu_expr_params.py (its RULES and their derivation), with the multiplier a field: A = c0 + c1
# f(f[0] * arg) where f[0] is 1 or 2 from cell to cell -- a power of two, so f[0] * arg is exact, and the tangent of the product,
# add(mul(f[0], 0), mul(1, arg)) = arg, is exact: host and device apply the rule of f to the same bits a = f[0] arg, da = arg.
def _rules():
    import test_gpu_expr_params as GP

    return GP.RULES


@pytest.mark.parametrize("f", list(G.FUNCTIONS))
@pytest.mark.parametrize("name", FUNCTION_SHAPES)
def test_tangents_of_a_math_function_are_within_its_ulps(name, f):
    c0, c1, arg = G.FUNCTIONS[f]
    A = E(f"{c0} + {c1}*{f}(f[0]*({arg}))", fields=1)
    nc = SHAPES[name][3]
    # tan has a pole in the doubled argument (0.5 y + 0.25 x reaches 0.75: twice that passes pi / 2); its cells keep 1 and 0.5
    scale = np.where(np.arange(nc) % 2 == 0, 1.0, 0.5 if f == "tan" else 2.0)[:, None]
    rows = np.concatenate([G._midpoints(nc), scale], axis=1)
    stream, yq, w, _ = _stream(name, A, rows)
    arg_v = E(arg).components(rows.T[:3, :, None, None], np.moveaxis(yq, -1, 0)[:, None])[0]  # [nc, n_el, n_q]
    a = scale[:, :, None] * arg_v
    g, K, term = _rules()[f]
    U = 0 if g is None else max(2, 2 * MEASURED_ULP[g])
    # the rule's term with a = f[0] arg and da = arg: term(a) of the params test is the term at da = a
    D = np.abs(term(a) / scale[:, :, None]).max()
    tol = abs(c1) * (K(U) + 2 + len(w)) * 2.0**-52 * np.abs(w).sum() * D
    coef, dirs = G._plan(name).expand_tangents(stream)
    host = A.host_tangents(rows, yq, w)
    err = np.abs(dirs - host).max()
    print(f"{name} {f}: max |device - host| of the tangent = {err:.3e}, tolerance {tol:.3e} (U = {U}, K = {K(U)}, n_q = {len(w)}, D = {D:.4f})")
    assert np.all(np.isfinite(host)) and np.abs(host).max() > 0.05
    assert err <= tol
    assert np.array_equal(coef, G._plan(name).expand(stream))  # the value part is the value pass's (k_expand_program<0>), whatever the functions


# -- 3. a field with one value in every cell is a parameter ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused5", "elasticity4", "poisson3d", "fused3x300"])
def test_equal_field_values_give_the_stream_and_tangents_of_the_parameter_bitwise(name):
    dim, _, kind, nc = SHAPES[name]
    z = "y[1]" if dim == 2 else "y[2]"
    text = f"1.5 + x[0] + p[0]*sin(2*pi*y[0])*{z} + sqrt(1 + p[0]*y[1]) + (p[0] + y[0])**2/(2 + p[0])"
    v = 0.6180339887
    shaped = lambda s, **kw: E(s, **kw) if kind == "poisson" else E(lam=s, mu=f"0.5*({s}) + 1", **kw)
    par, fld = shaped(text, p=[v]), shaped(text.replace("p[", "f["), fields=1)
    x = G._midpoints(nc)
    yq, w = G._points(name, par.degree)
    p = G._plan(name)
    sp = CoefStream.program(yq, w, *par.program(), par.n_comp, x, n_params=1)
    sf = CoefStream.program(yq, w, *fld.program(), fld.n_comp, np.concatenate([x, np.full((nc, 1), v)], axis=1), n_fields=1)
    (cp, dp), (cf, df) = p.expand_tangents(sp), p.expand_tangents(sf)
    assert np.array_equal(cf, cp) and np.array_equal(df, dp) and np.array_equal(p.expand(sf), p.expand(sp))
    assert np.all(np.isfinite(df)) and np.abs(df).max() > 0.1


# -- 4. position and chunking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("fused5", FOUR_FIELDS), ("elasticity4", TWO_AND_TWO), ("fused3x300", TWO_FIELDS)])
def test_permuting_the_cells_with_their_rows_permutes_every_output_bitwise(name, k):
    p = G._plan(name)
    stream, host, tangents = _case(name, k)
    nc = len(stream)
    perm = np.random.default_rng(41).permutation(nc)
    assert np.any(perm != np.arange(nc))
    moved = CoefStream(stream.method, stream.shared, np.ascontiguousarray(stream.per_cell[perm]))
    assert np.array_equal(p.expand(moved), host[perm])
    coef, dirs = p.expand_tangents(moved)
    assert np.array_equal(coef, host[perm]) and np.array_equal(dirs, tangents[perm])
    here, there = _families(p, stream, None, directions="parameters"), _families(p, moved, None, directions="parameters")
    for key in here:
        assert np.array_equal(there[key], here[key][perm]), key


def _families(p, coef, M, **dirs):
    s = p.sensitivities(coef, M, **dirs)
    s2 = p.second_sensitivities(coef, M, first=True, **dirs)
    return {"dA": s.dA, "A": s.A_eff, "info": s.info, "d2A": s2.d2A, "dA2": s2.dA, "A2": s2.A_eff, "info2": s2.info}


CHUNK_CELLS = 60  # a fused n = 5 cell holds 43 KB of factor record, refinement scratch and correctors: 1 MB takes some 20 of them


def _chunk_case():
    A = _expression("poisson", 2, TWO_AND_TWO)
    stream, yq, w, rows = _stream("fused5", A, _rows(CHUNK_CELLS, A.n_fields, seed=31))
    M = np.eye(2)[None] + 0.2 * np.random.default_rng(33).uniform(-1.0, 1.0, (CHUNK_CELLS, 2, 2))
    p = G._plan("fused5")
    out = _families(p, stream, M, directions="parameters")
    r = p.reconstruct(stream, np.random.default_rng(35).standard_normal((CHUNK_CELLS, p.t)), M, fields=True)
    out.update(strain=r.strain, flux=r.flux, energy=r.energy)
    return out, (A, rows, yq, w, M)


def test_field_directions_do_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the same calls in chunks of 1 MB, each of which
    must find the rows of its own cells."""
    here, (A, rows, yq, w, M) = _chunk_case()
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, HOMMX_RECON_MEM_MB="1"), timeout=300)
    child = np.load(out)
    for key in here:
        assert np.array_equal(child[key], here[key]), key
    assert not here["info"].any() and np.all(np.isfinite(here["d2A"]))
    want = _families(G._plan("fused5"), A.host_stream(rows, yq, w), M, directions=A.host_tangents(rows, yq, w), per_cell=True)
    for key in want:  # and both are what the sampled stream and tangents give
        assert np.array_equal(here[key], want[key]), key


# -- 5. the derived families -------------------------------------------------------------------------------------------------------------
def _families_device(p, stream, M, n_tan):
    """Sensitivities and second sensitivities through the device entries with per_cell="parameters", and the reconstruction."""
    import torch

    dev = torch.device("cuda", p.device)
    keep = []
    upload = _uploader(dev, keep)
    nc, t = len(stream), p.t
    st = torch.cuda.current_stream(dev).cuda_stream
    new = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device=dev)
    dA, A, d2A, dA2, A2 = new(nc, n_tan, t, t), new(nc, t, t), new(nc, n_tan, n_tan, t, t), new(nc, n_tan, t, t), new(nc, t, t)
    info, info2 = (torch.full((nc,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    src = stream.coef_source(upload)
    Mp = None if M is None else upload(M)
    p.sensitivities_device(nc, src, Mp, n_tan, None, "parameters", dA.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(), stream=st)
    p.second_sensitivities_device(nc, src, Mp, n_tan, None, d2A.data_ptr(), "parameters", dA2.data_ptr(), A2.data_ptr(), info2.data_ptr(), st)
    xi = _xi(nc, t)
    stats, strain, flux = new(nc, 2 * t + 3), new(nc, p.n_el, t), new(nc, p.n_el, t)
    p.reconstruct_source_device(nc, src, Mp, upload(xi), stats.data_ptr(), strain_ptr=strain.data_ptr(), flux_ptr=flux.data_ptr(), stream=st)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in dict(dA=dA, A=A, info=info, d2A=d2A, dA2=dA2, A2=A2, info2=info2, stats=stats, strain=strain,
                                                 flux=flux).items()}


def _xi(nc, t):
    return np.random.default_rng(37).standard_normal((nc, t))


def _host_families(p, coef, M, **dirs):
    out = _families(p, coef, M, **dirs)
    r = p.reconstruct(coef, _xi(len(coef), p.t), M, fields=True)
    out.update(stats=np.concatenate([r.mean_strain, r.mean_flux, r.energy[:, None], r.max_flux[:, None], r.argmax_element[:, None]], axis=1),
               strain=r.strain, flux=r.flux)
    return out


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("name,k", [("fused5", FOUR_FIELDS), ("elasticity4", TWO_AND_TWO), ("mesh", TWO_AND_TWO), ("fused3x300", TWO_FIELDS)])
def test_derived_families_equal_the_sampled_stream_and_tangents_bitwise(name, k, with_M):
    p = G._plan(name)
    stream, host, tangents = _case(name, k)
    M = G._M(name) if with_M else None
    want = _host_families(p, host, M, directions=tangents, per_cell=True)
    assert not want["info"].any() and not want["info2"].any()
    assert all(np.all(np.isfinite(v)) for v in want.values()) and np.abs(want["d2A"]).max() > 0
    got = _host_families(p, stream, M, directions="parameters")
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    got = _families_device(p, stream, M, tangents.shape[1])
    for key in want:
        assert np.array_equal(got[key], want[key]), ("device", key)


# -- 6. end to end, Poisson --------------------------------------------------------------------------------------------------------------
def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


STEP = 1e-5  # step and tolerance of test_gpu_expr_params.py::test_poisson_hmm_end_to_end: the same kernels against the same kind of difference


def test_poisson_hmm_end_to_end(caplog):
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(8, 8)
    h = hmm.PoissonHMM(msh, E("1.1 + x[0] + f[0]*sin(2*pi*y[0]) + f[1]*y[1]*(1-y[1])", fields=2), lambda x: 1.0 + x[0], micro, 0.01)
    assert h._coeff.affine_in_parameters
    with pytest.raises(RuntimeError, match="set_fields"):
        h.solve()
    with pytest.raises(RuntimeError, match="set_fields"):
        h.tensor_derivatives()
    f0 = np.random.default_rng(43).uniform(0.2, 0.6, (msh.num_cells, 2)) * np.array([1.0, 4.0])
    h.set_fields(f0)
    u = h.solve().x.array.copy()
    plan = h._plan
    assert hasattr(plan, "solve_program") and not h.cell_info.any()
    A0, K0 = h.effective_tensors.copy(), h._A.copy()
    r = h.tensor_derivatives()
    assert r.names == ("f0", "f1") and r.dA.shape == (msh.num_cells, 2, 2, 2) and not r.info.any()
    _close(r.A_eff, A0, 1e-12, "A_eff of the corrector route against the tensor route")
    e = h.energy_derivatives()
    s2 = h.tensor_second_derivatives()
    assert s2.names == ("f0", "f1") and s2.d2A.shape == (msh.num_cells, 2, 2, 2, 2) and np.array_equal(s2.dA, r.dA)
    assert e.shape == (msh.num_cells, 2)
    assert not [rec for rec in caplog.records if rec.levelname == "WARNING"]
    for T in (3, 20):
        others = np.delete(np.arange(msh.num_cells), T)
        fd2 = np.empty((2, 2, 2, 2))
        for k in range(2):
            side = []
            for sign in (+1.0, -1.0):
                q = f0.copy()
                q[T, k] += sign * STEP
                h.set_fields(q)
                assert h._needs_reassembly and h._plan is plan
                h.solve()  # reassembles: the tensors and the macro matrix at q
                assert not h._needs_reassembly and h._plan is plan and not h.cell_info.any()
                assert np.array_equal(h.effective_tensors[others], A0[others])  # no other cell reads the row of T
                side.append((h.effective_tensors[T].copy(), h._A.copy(), h.tensor_derivatives(cells=[T]).dA[0]))
            (Ap, Kp, dp), (Am, Km, dm) = side
            assert np.abs(Ap - Am).max() > 0
            _close(r.dA[T, k], (Ap - Am) / (2 * STEP), 1e-6, f"d A_H[{T}] / d f{k}[{T}] against central differences")
            fd_e = (u @ (Kp @ u) - u @ (Km @ u)) / (2 * STEP)
            err = abs(e[T, k] - fd_e) / abs(fd_e)  # the ENTRY, not a sum over cells: the whole derivative with respect to (T, k)
            print(f"d (u . K_H u) / d f{k}[{T}] against central differences", err)
            assert err < 1e-6
            fd2[:, k] = (dp - dm) / (2 * STEP)
        _close(s2.d2A[T], fd2, 1e-6, f"d2 A_H[{T}] / df df against central differences of dA")
    h.set_fields(f0)
    assert np.array_equal(h.tensor_derivatives(cells=[3, 20]).dA, r.dA[[3, 20]])
    h.solve()
    assert np.array_equal(h.effective_tensors, A0) and np.array_equal(h._A.toarray(), K0.toarray())


# -- 7. end to end, elasticity -----------------------------------------------------------------------------------------------------------
def test_linear_elasticity_hmm():
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(4, 4)
    h = hmm.LinearElasticityHMM(msh, E(lam="1.25", mu="5 + f[0]*sin(2*pi*y[0])", fields=1), lambda x: np.zeros(2), micro, 0.01)
    f0 = np.random.default_rng(47).uniform(3.5, 4.5, msh.num_cells)
    h.set_fields(f0)  # one field: a 1-D array
    r = h.tensor_derivatives()
    assert r.names == ("f0",) and r.dA.shape == (msh.num_cells, 1, 3, 3) and r.A_eff.shape == (msh.num_cells, 3, 3) and not r.info.any()
    s2 = h.tensor_second_derivatives()
    assert s2.d2A.shape == (msh.num_cells, 1, 1, 3, 3) and np.array_equal(s2.dA, r.dA)
    h._assemble_stiffness()
    A0 = h.effective_tensors.copy()
    for T in (3, 20):
        side = []
        for sign in (+1.0, -1.0):
            q = f0.copy()
            q[T] += sign * STEP
            h.set_fields(q)
            h._assemble_stiffness()
            assert not h.cell_info.any()
            assert np.array_equal(np.delete(h.effective_tensors, T, axis=0), np.delete(A0, T, axis=0))
            side.append((h.effective_tensors[T].copy(), h.tensor_derivatives(cells=[T]).dA[0, 0]))
        _close(r.dA[T, 0], (side[0][0] - side[1][0]) / (2 * STEP), 1e-6, f"d C_H[{T}] / d f0[{T}] against central differences")
        _close(s2.d2A[T, 0, 0], (side[0][1] - side[1][1]) / (2 * STEP), 1e-6, f"d2 C_H[{T}] / d f0 d f0 against central differences of dA")


# -- 8. a solution-dependent coefficient -------------------------------------------------------------------------------------------------
def test_fields_from_a_callable_and_a_picard_loop():
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(8, 8)
    rhs = lambda x: 1.0 + x[0]
    # g(x) written out in x and the same g as a field: both programs hold exactly rounded operations only, and NumPy forms g with the
    # operations the program spells (a product, then a sum), so the device multiplies the same bits by y either way
    a = hmm.PoissonHMM(msh, E("1.5 + (0.25 + x[0]*x[1])*y[0]*(1 - y[0]) + (0.5 - 0.25*x[1])*y[1]"), rhs, micro, 0.01)
    b = hmm.PoissonHMM(msh, E("1.5 + f[0]*y[0]*(1 - y[0]) + f[1]*y[1]", fields=2), rhs, micro, 0.01)
    b.set_fields(lambda x: np.stack([0.25 + x[0] * x[1], 0.5 - 0.25 * x[1]]))
    assert len(np.unique(b._fields, axis=0)) == msh.num_cells  # every cell has a row of its own
    a._assemble_stiffness()
    b._assemble_stiffness()
    assert hasattr(b._plan, "solve_program") and not b.cell_info.any()
    assert np.array_equal(b.effective_tensors, a.effective_tensors)
    # two Picard steps of A(x, u_H(x), y) = 1.5 + x[0] + u sin(2 pi y[0])^2, the field fed from the last solution, against the same loop
    # on a callable sampled on the host, which looks its u up by the cell of the midpoint it is given
    h = hmm.PoissonHMM(msh, E("1.5 + x[0] + f[0]*sin(2*pi*y[0])**2", fields=1), rhs, micro, 0.01)
    mid = msh.cell_midpoints()
    u_host = np.zeros(msh.num_cells)

    def sampled(x, y):
        x = np.asarray(x)
        cells = np.argmin(((x[:2].reshape(2, -1, 1) - mid[:, :2].T[:, None, :]) ** 2).sum(axis=0), axis=1).reshape(x[0].shape)
        return 1.5 + x[0] + u_host[cells] * np.sin(2 * np.pi * y[0]) ** 2

    g = hmm.PoissonHMM(msh, sampled, rhs, micro, 0.01, quadrature_degree=h.quadrature_degree_used)
    h.set_fields(np.zeros(msh.num_cells))
    h.solve()
    g.solve()
    plan = h._plan
    for step in range(2):
        u = h.cell_means()
        assert u.shape == (msh.num_cells,) and len(np.unique(u)) > msh.num_cells // 2
        h.set_fields(u)
        assert h._needs_reassembly and h._plan is plan
        h.solve()
        assert h._plan is plan and not h.cell_info.any()
        u_host[:] = g.cell_means()
        g._needs_reassembly = True  # the callable reads the new u
        g.solve()
        err = np.abs(h.effective_tensors - g.effective_tensors).max(axis=(1, 2)) / np.abs(g.effective_tensors).max(axis=(1, 2))
        print(f"Picard step {step}: max relative difference per cell tensor, device-sampled fields against host sampling: {err.max():.3e}")
        assert err.max() < 1e-10
    assert np.abs(h.effective_tensors - b.effective_tensors).max() > 1e-3  # and the loop went somewhere

if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case()[0])
