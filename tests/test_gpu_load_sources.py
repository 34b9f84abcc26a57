"""Loads sampled on the device on an MI355X (-m gpu): hommx_loads_source[_device] with HOMMX_LOADS_PROGRAM (the load is the program of a
vector ``Expression``) and HOMMX_LOADS_EIGENSTRAIN (what arrives is an eigenstrain; k_eigenstress forms P = -material(coef) E), on the
small plans of tests/test_gpu_loads.py, NC = 5 cells.

Bitwise where the arithmetic is exact: a program of exactly rounded operations against the per-cell path fed with its own host stream;
an eigenstrain whose coefficient and values are integer multiples of 2^-3 below 8 -- every product and partial sum of material(coef) E
is then exact in fp64 in any order, fused or not -- against the per-cell path fed with the reference's -C : E.  Against the NumPy /
SciPy reference (tests/loads_ref.py) at the 1e-10 (per-cell reductions) / 1e-9 (correctors and fields) of test_gpu_loads.py.  Device
entry against host entry, chunking and the stream order (tests/stream_order_gpu.py) bitwise.  The solver classes at ten times the
difference between the host interpreter and the hand-written callable that tests/test_load_sources_hmm_host.py measures on the CPU."""

import contextlib
import functools
import os

import numpy as np
import pytest

import load_sources_cases as S
import loads_ref as L
from hommx_amd import MicroCellPlan, _lib, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream, Program
from hommx_amd.expr import Expression

pytestmark = pytest.mark.gpu

# name -> (dim, n or None on the jittered mesh, kind, route of from_mesh): the small cases of test_gpu_loads.py
CASES = {
    "fused_16": (2, 8, "poisson", None),  # NB = 16
    "fused_32": (2, 20, "poisson", None),  # 800 elements: more than one per thread
    "small_wave_2d": (2, 6, "elasticity", None),
    "multifrontal": (3, 5, "elasticity", None),  # t = 6 = PROGRAM_MAX_COMP, 750 elements
    "mesh_tree_3d": (3, None, "poisson", "tree"),
    "mesh_front": (2, None, "elasticity", None),  # P_eff alone: the load solve is refused
}
# the kinds those cases do not have, for k_eigenstress: a symmetric matrix, and the full Voigt matrix in 2D (3 x 3) and 3D (6 x 6)
KIND_CASES = {"matrix_2d": (2, 6, "poisson_matrix", None), "voigt_2d": (2, 6, "elasticity_voigt", None), "voigt_3d": (3, 4, "elasticity_voigt", None)}
ALL = {**CASES, **KIND_CASES}
NC = 5


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@functools.lru_cache(maxsize=None)
def _micro(name):
    """The mesh whose element order the plan of `name` has."""
    dim, n = ALL[name][:2]
    if n is None:
        return W.jittered_unit_square(10, 8) if dim == 2 else W.jittered_unit_cube(4, 4, 4)
    return Mm.create_unit_square(n, n) if dim == 2 else Mm.create_unit_cube(n, n, n)


@functools.lru_cache(maxsize=None)
def _plan(name, recon_mb=None):
    dim, n, kind, route = ALL[name]
    with _environment({"HOMMX_RECON_MEM_MB": str(recon_mb)} if recon_mb else {}):
        return MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(_micro(name), kind, route=route)


@functools.lru_cache(maxsize=None)
def _points(name, degree):
    """(yq[n_el, n_q, dim], w[n_q]) of the rule of `degree` on the elements of the plan; degree 1 is the centroid rule, one point of weight 1."""
    bary, w = hmm.micro_quadrature(ALL[name][0], degree)
    yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, _micro(name).cell_vertices()))
    for a in (yq, w):
        a.setflags(write=False)
    return yq, np.ascontiguousarray(w)


@functools.lru_cache(maxsize=None)
def _case(name):
    """NC cells with distinct coefficients and M, the rows of a load program (midpoints in [0, 1]^3, then two fields that are integer
    multiples of 2^-3 in [-3, 3]) and the reference cells; computed once, read only."""
    dim, n, kind, _ = ALL[name]
    p = _plan(name)
    rng = np.random.default_rng(sorted(ALL).index(name))
    coef = np.stack([L.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([L.random_M(dim, rng) for _ in range(NC)])
    rows = np.ascontiguousarray(np.concatenate([rng.uniform(0.0, 1.0, (NC, 3)), rng.integers(-24, 25, (NC, 2)) / 8.0], axis=1))
    refs = [L.structured(kind, dim, n, coef[k], M[k]) if n else L.on_mesh(_micro(name), kind, coef[k], M[k], p.to_periodic) for k in range(NC)]
    for a in (coef, M, rows):
        a.setflags(write=False)
    return coef, M, rows, refs


def _kw(name):
    return {} if name == "mesh_front" else {"fields": True, "return_correctors": True}


def _fields_of(r):
    return {k: v for k, v in vars(r).items() if v is not None}


def _assert_equal(a, b):
    """np.array_equal on every output: P_eff, A_eff, info, energy, the stats (mean and max flux, its element), strain, flux, correctors."""
    fa, fb = _fields_of(a), _fields_of(b)
    assert fa.keys() == fb.keys() and {"P_eff", "A_eff", "info"} <= fa.keys()
    for key in fa:
        assert np.array_equal(fa[key], fb[key], equal_nan=True), key


def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


def _stream(A, name, rows, degree):
    yq, w = _points(name, degree)
    return CoefStream.program(yq, w, *A.program(), A.n_comp, rows[:, :3 + A.n_fields], n_params=A.n_params, n_fields=A.n_fields)


def _exact_load(t, dim):
    """A load program of exactly rounded operations only: where, + - * /, x, y, one parameter, one field."""
    return Expression([f"where(y[{c % dim}] < 0.5, p[0]*x[{c % 3}] + f[0], y[{(c + 1) % dim}]/({c} + 1.5)) - x[1]*y[{c % dim}]" for c in range(t)],
                      p=[0.75], fields=1)


def _exact_strain(t, dim):
    """An eigenstrain program whose values at any point are integer multiples of 2^-3 below 8 when its fields are such multiples in
    [-3, 3] (the rows of ``_case``); under the centroid rule (one point of weight 1) its element means are those values."""
    return Expression([f"where(y[{c % dim}] < 0.5, p[0]*f[0], 0.25 - f[1])" if c % 2 == 0 else f"where(y[{(c + 1) % dim}] < 0.25, -f[1], f[0] + 0.5)"
                       for c in range(t)], p=[2.0], fields=2)


# -- 1. a program load against its own stream ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_program_load_equals_the_per_cell_path_fed_with_its_host_stream(name):
    p = _plan(name)
    coef, M, rows, _ = _case(name)
    A = _exact_load(p.t, p.dim)
    yq, w = _points(name, 2)
    P = A.host_stream(rows[:, :4], yq, w)  # [NC, n_el, t]
    assert P.shape == (NC, p.n_el, p.t) and np.isfinite(P).all()
    want = p.loads(coef, P[:, None], M, per_cell=True, **_kw(name))
    assert not want.info.any()
    _assert_equal(p.loads(coef, _stream(A, name, rows, 2), M, **_kw(name)), want)
    with pytest.raises(ValueError, match="n_comp == t"):
        p.loads(coef, _stream(_exact_load(p.t + 1, p.dim), name, rows, 2) if p.t < 6 else _stream(_exact_load(p.t - 1, p.dim), name, rows, 2), M)
    with pytest.raises(ValueError, match="rows of the load"):
        p.loads(coef[:3], _stream(A, name, rows, 2), M[:3])


# -- 2. an eigenstrain against the per-cell path, exactly -----------------------------------------------------------------------------------
def _eighths(rng, lo, hi, shape):
    return rng.integers(lo, hi, shape) / 8.0


def _exact_coef(kind, dim, n_el, rng):
    """SPD coefficient values that are integer multiples of 2^-3 below 8 (diagonally dominant where there is a matrix)."""
    t = L.tensor_size(kind, dim)
    if kind == "poisson":
        return _eighths(rng, 1, 64, n_el)
    if kind == "elasticity":
        return _eighths(rng, 1, 64, (n_el, 2))
    if kind == "poisson_matrix":  # (00, 11[, 22], 01[, 02, 12])
        return np.concatenate([_eighths(rng, 32, 64, (n_el, dim)), _eighths(rng, -8, 9, (n_el, t * (t + 1) // 2 - dim))], axis=1)
    iu = np.triu_indices(t)  # the upper triangle of the t x t matrix, row-major: five off-diagonal entries of at most 1 against 6
    return np.where(iu[0] == iu[1], _eighths(rng, 48, 64, (n_el, len(iu[0]))), _eighths(rng, -8, 9, (n_el, len(iu[0]))))


@functools.lru_cache(maxsize=None)
def _exact_case(name):
    dim, n, kind, _ = ALL[name]
    p = _plan(name)
    rng = np.random.default_rng(50 + sorted(ALL).index(name))
    coef = np.stack([_exact_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    V = np.stack([L.voigt_material(kind, coef[k], dim, p.n_el) for k in range(NC)])  # the reference's material matrix, [NC, n_el, t, t]
    assert np.array_equal(V * 32, np.round(V * 32)) and np.array_equal(V, hmm.material_matrix(coef, kind, dim))  # exact, and the host helper's
    M = _case(name)[1] if name in CASES else np.stack([L.random_M(dim, rng) for _ in range(NC)])
    shared, per_cell = _eighths(rng, -63, 64, (p.t, p.n_el, p.t)), _eighths(rng, -63, 64, (NC, p.t, p.n_el, p.t))
    for a in (coef, V, shared, per_cell):
        a.setflags(write=False)
    return coef, M, V, shared, per_cell


def _stress(V, E):
    """NumPy's -C : E per cell: E[NC, n_loads, n_el, t] or, shared, [n_loads, n_el, t]."""
    return -np.einsum("cemn,clen->clem", V, np.broadcast_to(E, (NC,) + E.shape[-3:]))


@pytest.mark.parametrize("name", list(ALL))
def test_eigenstrain_equals_the_per_cell_path_fed_with_the_eigenstress(name):
    p = _plan(name)
    coef, M, V, shared, per_cell = _exact_case(name)
    kw = _kw(name)
    for E in (per_cell, per_cell[:, :1], shared, shared[1:2]):
        want = p.loads(coef, _stress(V, E), M, per_cell=True, **kw)
        assert not want.info.any() and np.isfinite(want.P_eff).all()
        _assert_equal(p.loads(coef, E, M, eigenstrain=True, **kw), want)
    # E from a program, under the centroid rule
    A, rows = _exact_strain(p.t, p.dim), _case(sorted(CASES)[0])[2]
    yq, w = _points(name, 1)
    assert w.tolist() == [1.0]
    E = A.host_stream(rows, yq, w)[:, None]
    assert np.array_equal(E * 8, np.round(E * 8)) and np.abs(E).max() < 8 and len(np.unique(E)) > 8
    _assert_equal(p.loads(coef, _stream(A, name, rows, 1), M, eigenstrain=True, **kw), p.loads(coef, _stress(V, E), M, per_cell=True, **kw))


# -- 3. against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_eigenstrain_matches_reference(name):
    p = _plan(name)
    coef, M, _, refs = _case(name)
    yb = _points(name, 1)[0][:, 0, :]  # element barycentres
    E = np.stack([np.stack([np.sin(2 * np.pi * yb[:, k % p.dim] + c) + 0.3 * k + 0.1 * c for k in range(p.t)], axis=-1) for c in range(NC)])[:, None]
    r = p.loads(coef, E, M, eigenstrain=True, **_kw(name))
    assert not r.info.any()
    for k, ref in enumerate(refs):
        P = -np.einsum("emn,len->lem", ref.V, E[k])
        if name == "mesh_front":
            _close(r.P_eff[k], ref.levin(P), 1e-10, f"{name} cell {k} P_eff")
            _close(r.A_eff[k], ref.A, 1e-10, f"{name} cell {k} A_eff")
            continue
        want = ref.solve(P)
        _close(r.P_eff[k], want["P_eff"], 1e-10, f"{name} cell {k} P_eff (Levin)")
        _close(r.mean_flux[k], want["P_eff"], 1e-10, f"{name} cell {k} mean total flux")
        _close(r.energy[k], want["energy"], 1e-10, f"{name} cell {k} energy")
        _close(r.max_flux[k], want["max_flux"], 1e-10, f"{name} cell {k} max flux")
        _close(r.A_eff[k], ref.A, 1e-10, f"{name} cell {k} A_eff")
        _close(r.correctors[k], want["chi"], 1e-9, f"{name} cell {k} correctors")
        _close(r.strain[k], want["eps"], 1e-9, f"{name} cell {k} strain")
        _close(r.flux[k], want["q"], 1e-9, f"{name} cell {k} flux")


@pytest.mark.parametrize("name", list(CASES))
def test_uniform_eigenstrain_in_a_homogeneous_cell(name):
    """A homogeneous coefficient with a uniform E: the load is divergence free, the corrector vanishes, P_eff = -C E, and the energy is
    zero at the scale E . C E of the energy a field of that size could store (1e-10 of it, the tolerance of the reductions)."""
    dim, n, kind, _ = CASES[name]
    p = _plan(name)
    rng = np.random.default_rng(7)
    one = np.stack([L.random_coef(kind, dim, 1, rng)[0] for _ in range(NC)])  # one value per cell
    coef = np.ascontiguousarray(np.broadcast_to(one[:, None], (NC, p.n_el) + one.shape[1:]))
    E0 = rng.standard_normal((NC, p.t))
    E = np.ascontiguousarray(np.broadcast_to(E0[:, None, None, :], (NC, 1, p.n_el, p.t)))
    r = p.loads(coef, E, _case(name)[1], eigenstrain=True, response=name != "mesh_front")
    C = np.stack([L.voigt_material(kind, one[k], dim, 1)[0] for k in range(NC)])
    assert not r.info.any()
    _close(r.P_eff[:, 0], -np.einsum("cmn,cn->cm", C, E0), 1e-10, f"{name} P_eff = -C E")
    if name != "mesh_front":
        scale = np.einsum("cm,cmn,cn->c", E0, C, E0)
        print(name, "energy over E . C E", np.abs(r.energy[:, 0, 0] / scale).max())
        assert (np.abs(r.energy[:, 0, 0]) < 1e-10 * scale).all()


# -- 4. the device entry against the host entry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("code", [2, 4, 5, 6])
def test_device_entry_equals_host_entry(name, code):
    import torch

    p = _plan(name)
    coef, M, V, shared, per_cell = _exact_case(name)
    rows = _case(name)[2]
    solved = name != "mesh_front"
    eigenstrain = bool(code & _lib.LOADS_EIGENSTRAIN)
    if code & 3 == _lib.LOADS_PROGRAM:
        load = _stream(_exact_strain(p.t, p.dim), name, rows, 1) if eigenstrain else _stream(_exact_load(p.t, p.dim), name, rows, 2)
        nl = 1
    else:
        load = per_cell if code & 1 else shared
        nl = p.t
    want = p.loads(coef, load, M, eigenstrain=eigenstrain, fields=solved, return_correctors=solved)
    assert not want.info.any()
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))  # a copy: the cached case is read only
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    t = p.t
    out = {"P_eff": empty(NC, nl, t), "A_eff": empty(NC, t, t), "info": empty(NC, dtype=torch.int32)}
    if solved:
        out.update(energy=empty(NC, nl, nl), stats=empty(NC, nl, t + 2), strain=empty(NC, nl, p.n_el, t), flux=empty(NC, nl, p.n_el, t),
                   correctors=empty(NC, nl, want.correctors.shape[2]))
    ptr = lambda key: out[key].data_ptr() if key in out else None
    program = isinstance(load, CoefStream)
    P_ptr = None if program else upload(load)
    given = None if program else keep[-1]
    p.loads_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nl, P_ptr, ptr("P_eff"), bool(code & 1), ptr("A_eff"), ptr("info"),
                   ptr("energy"), ptr("stats"), ptr("strain"), ptr("flux"), ptr("correctors"), stream=torch.cuda.current_stream(dev).cuda_stream,
                   eigenstrain=eigenstrain, P_source=load.coef_source(upload) if program else None)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for key in ("P_eff", "A_eff", "info") + (("energy", "strain", "flux", "correctors") if solved else ()):
        assert np.array_equal(got[key], getattr(want, key)), key
    if solved:
        assert np.array_equal(got["stats"][:, :, :t], want.mean_flux) and np.array_equal(got["stats"][:, :, t], want.max_flux)
        assert np.array_equal(got["stats"][:, :, t + 1], want.argmax_element)
    if given is not None:  # the caller's eigenstrain is an input: the device entry leaves it as it is
        assert np.array_equal(given.cpu().numpy(), load)


# -- 5. chunking ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_outputs_do_not_depend_on_chunking(name):
    """HOMMX_RECON_MEM_MB = 1 on a second plan, an eigenstrain from a program (code 6) on a two-phase coefficient source.  A chunk holds,
    among the rest, the fields [2][n_el][t] of the response (the expansion [n_el][t] of the load on a P_eff call), so twice the cells
    whose share of that fills 1 MB, and one more, make three chunks or more."""
    dim, n, kind, _ = CASES[name]
    p, small = _plan(name), _plan(name, 1)
    solved = name != "mesh_front"
    nc = 2 * max(1, (1 << 20) // (8 * (2 if solved else 1) * p.n_el * p.t)) + 1
    rng = np.random.default_rng(5)
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([L.random_coef(kind, dim, 2, rng) for _ in range(nc)])
    M = np.stack([L.random_M(dim, rng) for _ in range(nc)])
    rows = np.concatenate([rng.uniform(0.0, 1.0, (nc, 3)), rng.uniform(-3.0, 3.0, (nc, 2))], axis=1)
    coef, load = CoefStream.two_phase(mask, values), _stream(_exact_strain(p.t, p.dim), name, rows, 2)
    want = p.loads(coef, load, M, eigenstrain=True, **_kw(name))
    assert not want.info.any() and np.isfinite(want.P_eff).all()
    _assert_equal(small.loads(coef, load, M, eigenstrain=True, **_kw(name)), want)
    for k in (0, nc // 2, nc - 1):  # a cell alone: its position in the batch and in the chunk does not matter either
        one = p.loads(coef.block(k, k + 1), load.block(k, k + 1), M[k:k + 1], eigenstrain=True)
        assert np.array_equal(one.P_eff[0], want.P_eff[k])


# -- 6. the stream order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused2d_32", "mesh_tree"])  # a fused plan and a tree plan
@pytest.mark.parametrize("code", [2, 6])
def test_stream_order(name, code):
    """The in-flight protocol of tests/stream_order_gpu.py on hommx_loads_source_device with a program load: the coefficient, M, and the
    points, weights and rows of the load program hold decoys until the stream brings the real ones -- decoy rows are a decoy load or
    a decoy eigenstrain --, `ready` is still unset when the call returns, and every kept output equals the synchronous reference."""
    import stream_order_gpu as H

    dim, n = H.PLANS[name][:2]
    p = H.plan(name)
    nc = 40 if name == "mesh_tree" else 24  # the cells of test_gpu_stream_order.py for these plans
    micro = H.mesh(dim) if n is None else Mm.create_unit_square(n, n)
    bary, w = hmm.micro_quadrature(dim, 2)
    yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, micro.cell_vertices()))
    A = _exact_strain(p.t, dim) if code & _lib.LOADS_EIGENSTRAIN else _exact_load(p.t, dim)
    ops, consts = A.program()
    prog = Program(np.ascontiguousarray(ops), np.ascontiguousarray(consts), A.n_comp, A.n_params, A.n_fields)
    g = prog.struct()

    def inputs(seed):
        rng = np.random.default_rng(900 + seed)
        rows = np.concatenate([rng.uniform(0.0, 1.0, (nc, 3)), rng.uniform(-3.0, 3.0, (nc, A.n_fields))], axis=1)
        # the decoy points are the real ones shifted inside the cell: another valid rule
        return dict(H.inputs(name, nc, seed), rows=np.ascontiguousarray(rows), points=np.ascontiguousarray(yq if seed == 1 else 0.5 * yq + 0.125),
                    wq=np.ascontiguousarray(w if seed == 1 else w[::-1] * 0.5))

    def invoke(a, st):
        import ctypes as C

        src = _lib.CoefSource(form=_lib.COEF_PROGRAM, n_q=int(yq.shape[1]), table=a["points"], weights=a["wq"], params=a["rows"], program=C.pointer(g))
        src.n_fields = A.n_fields
        p.loads_device(nc, H._source(a, "sampled"), a["M"], 1, None, a["P_eff"], False, a["A_eff"], a["info"], a.get("energy"), a.get("stats"),
                       None, None, a.get("correctors"), st, eigenstrain=bool(code & _lib.LOADS_EIGENSTRAIN), P_source=src)

    bs = 1 if p.kind.startswith("poisson") else p.dim
    out = dict(H._tensor_outputs(p, nc), P_eff=((nc, 1, p.t), H.F64), energy=((nc, 1, 1), H.F64), stats=((nc, 1, p.t + 2), H.F64),
               correctors=((nc, 1, p.n_nodes * bs), H.F64))
    call = H.Call(f"loads code {code}", p, inputs(1), inputs(2), ("coef", "M", "rows", "points", "wq"), out, invoke)
    real, _ = H.references(call)
    H.in_flight(call, real, 100.0)  # DELAY_MS of test_gpu_stream_order.py, which derives it


# -- 7. the solver classes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_solver_class_eigenstrain_expression_against_the_callable(kind):
    """``set_eigenstrain(Expression([...], fields=("dT",)))`` with ``set_polarisation_fields`` against ``set_polarisation`` of the
    hand-written callable -A : E, on a ``TwoPhase`` coefficient (PoissonHMM 4 x 4 macro cells of 8 x 8; LinearElasticityStratifiedHMM 2 x 2
    of 6 x 6), in u and in the effective polarisation.  Tolerance: ten times the difference between the host interpreter of the
    expression and that callable on the CPU -- measured there as 0 and 1.9e-16, recorded as one unit roundoff 2.2e-16
    (load_sources_cases.CPU_DIFFERENCE) --, so 2.2e-15, far inside the 1e-9 / 1e-10 of the shift-identity tests."""
    h, E, P, g, _ = S.PROBLEMS[kind]()
    h.set_polarisation(P)
    u_want, P_want = S.solve(h, g), h.effective_polarisation.copy()
    plan = h._plan
    assert not h.cell_info.any() and plan.kernel == ("fused2d" if kind == "poisson" else "small_wave")
    h.set_eigenstrain(E)
    with pytest.raises(RuntimeError, match="set_polarisation_fields"):
        h.solve()
    h.set_polarisation_fields(S.fields(h))
    u, P_eff = S.solve(h, g), h.effective_polarisation.copy()
    assert h._plan is plan and not h.cell_info.any()
    tol = 10 * S.CPU_DIFFERENCE[kind]
    du, dP = S.difference(u, u_want), S.difference(P_eff, P_want)
    print(f"{kind}: u differs by {du:.3e}, P_eff by {dP:.3e}; tolerance {tol:.3e}")
    assert np.abs(P_want).max() > 1e-4 and du <= tol and dP <= tol
    # the response of the same load, and other parameters on the same plan
    r = h.load_response(cells=[0, 3], fields=True)
    _close(r.mean_flux[:, 0], P_eff[[0, 3]], 1e-10, f"{kind} load_response mean flux")
    if E.n_params:
        h.set_eigenstrain(E.with_parameters([-3.0]))
        S.solve(h, g)
        assert h._plan is plan and S.difference(h.effective_polarisation, P_want) > 1e-3
