"""The load solve of the frontal mesh route on an MI355X (-m gpu): plans of ``from_mesh(mesh, kind, route="front", load_solve=True)``
(HOMMX_MESH_FLAG_LOADS; load route "mesh_front_subst": k_mesh_front_rhs substitutes on the pivot columns of the corrector arena) on the
meshes of tests/stream_order_gpu.mesh -- the jittered 9 x 7 square and the jittered 3 x 4 x 3 cube --, every kind in 2D and 3D:

  routes        the three names of a flagged plan; the flag on the tree route changes nothing
  accuracy      hommx_loads_source against tests/loads_ref.py and against the tree-route plan of the same mesh, with and without M,
                n_loads in {1, t}, shared and per-cell P; the canonical loads as user loads; Levin's P_eff against the direct mean flux
  second        hommx_second_sensitivity_source against tests/sens2_ref.py, symmetric in (a, b) and (m, n) bitwise
  invariances   bitwise: batch position, chunking (HOMMX_RECON_MEM_MB = 1), outputs asked for, host against device entry, a load against
                the same load with others beside it
  failure       a cell with a non-positive coefficient keeps its info, its load rows are NaN, no other cell changes a bit
  stream order  the loads and the second-derivative device entries under the in-flight protocol of tests/stream_order_gpu.py
  end to end    PoissonHMM and LinearElasticityStratifiedHMM on a jittered micro mesh

Tolerances are those of tests/test_gpu_loads.py (1e-10 for per-cell reductions, 1e-9 for correctors and fields, relative to the largest
magnitude of the reference array of the cell) and of tests/test_gpu_sens2.py (TOL = 1e-9 of the cell's max |d2A|).

k_mesh_front_rhs keeps its vectors in global memory at every size: there is no size-dependent path to straddle.  It takes the front rows
of a pivot in segments of 32, eight (segment, load) items at a time: the fronts here are 18 / 23 unknowns wide for Poisson (one segment),
36 for 2D elasticity (two) and 69 for 3D elasticity (three; 18 items with t = 6 loads: more than one round of the eight half-waves), and
n_loads = 1 and t are the two ends of the item count."""

import functools
import os

import numpy as np
import pytest

import loads_ref as L
import sens2_ref as S2
import stream_order_gpu as H
from hommx_amd import MicroCellPlan, _lib, fem, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu

KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")
CASES = [(dim, kind) for dim in (2, 3) for kind in KINDS]
INVARIANT = [(2, "elasticity"), (3, "poisson"), (3, "elasticity_voigt")]  # bs = 2 / 1 / 3; t = 3 / 3 / 6
NC = 3
TOL2 = 1e-9  # tests/test_gpu_sens2.py, TOL


@functools.lru_cache(maxsize=None)
def _plan(dim, kind, route="front", recon_mb=None):
    old = os.environ.get("HOMMX_RECON_MEM_MB")
    if recon_mb:
        os.environ["HOMMX_RECON_MEM_MB"] = str(recon_mb)  # read when the plan is created
    try:
        return MicroCellPlan.from_mesh(H.mesh(dim), kind, route=route, load_solve=True)
    finally:
        if recon_mb:
            os.environ.pop("HOMMX_RECON_MEM_MB") if old is None else os.environ.__setitem__("HOMMX_RECON_MEM_MB", old)


@functools.lru_cache(maxsize=None)
def _case(dim, kind, strat=True):
    """NC cells with distinct coefficients (and M), t shared and t per-cell loads, and the reference cells; computed once, read only."""
    p = _plan(dim, kind)
    rng = np.random.default_rng(1000 * dim + 10 * KINDS.index(kind) + strat)
    coef = np.stack([L.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([L.random_M(dim, rng) for _ in range(NC)]) if strat else None
    shared = L.random_loads(rng, p.t, p.n_el, p.t)
    per_cell = np.stack([L.random_loads(rng, p.t, p.n_el, p.t) for _ in range(NC)])
    refs = [L.on_mesh(H.mesh(dim), kind, coef[k], None if M is None else M[k], p.to_periodic) for k in range(NC)]
    for a in (coef, shared, per_cell) + (() if M is None else (M,)):
        a.setflags(write=False)
    return coef, M, shared, per_cell, refs


def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


def _fields_of(r):
    return {k: v for k, v in vars(r).items() if v is not None}


def _assert_equal(a, b, cells=slice(None), other=slice(None)):
    fa, fb = _fields_of(a), _fields_of(b)
    assert fa.keys() == fb.keys()
    for key in fa:
        assert np.array_equal(fa[key][cells], fb[key][other], equal_nan=True), key


FULL = {"fields": True, "return_correctors": True}


# -- routes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_routes(dim):
    p = _plan(dim, "elasticity")
    assert (p.kernel, p.corrector_kernel, p.load_kernel) == ("mesh_front", "mesh_front", "mesh_front_subst")
    assert p.front_width > 0
    tree = _plan(dim, "elasticity", "tree")
    assert (tree.kernel, tree.corrector_kernel, tree.load_kernel) == ("mesh_multifrontal",) * 3 and tree.front_width == 0
    plain = MicroCellPlan.from_mesh(H.mesh(dim), "elasticity", route="front")
    assert (plain.kernel, plain.corrector_kernel, plain.load_kernel) == ("mesh_front", "mesh_front", "none")
    plain.close()


# -- accuracy --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [True, False])
@pytest.mark.parametrize("dim,kind", CASES)
def test_response_matches_reference_and_tree_route(dim, kind, strat):
    p, tree = _plan(dim, kind), _plan(dim, kind, "tree")
    coef, M, shared, per_cell, refs = _case(dim, kind, strat)
    for nl in (1, p.t):
        for P in (shared[:nl], per_cell[:, :nl]):
            what = f"{dim}D {kind} n_loads {nl} {'per cell' if P.ndim == 4 else 'shared'}"
            r, other = p.loads(coef, P, M, **FULL), tree.loads(coef, P, M, **FULL)
            assert r.P_eff.shape == (NC, nl, p.t) and r.energy.shape == (NC, nl, nl) and r.strain.shape == (NC, nl, p.n_el, p.t)
            assert r.correctors.shape == (NC, nl, other.correctors.shape[2]) and not r.info.any()
            assert np.array_equal(r.energy, np.swapaxes(r.energy, 1, 2))
            for k, ref in enumerate(refs):
                want = ref.solve(P[k] if P.ndim == 4 else P)
                _close(r.P_eff[k], want["P_eff"], 1e-10, f"{what} cell {k} P_eff (Levin)")
                _close(r.mean_flux[k], want["P_eff"], 1e-10, f"{what} cell {k} mean total flux")
                _close(r.P_eff[k], r.mean_flux[k], 1e-10, f"{what} cell {k} Levin against the device's direct mean flux")
                _close(r.energy[k], want["energy"], 1e-10, f"{what} cell {k} energy")
                _close(r.max_flux[k], want["max_flux"], 1e-10, f"{what} cell {k} max flux")
                for l in range(nl):  # the element the device names reaches the reference's maximum
                    assert want["norm"][l, r.argmax_element[k, l]] >= want["max_flux"][l] * (1 - 1e-9)
                _close(r.A_eff[k], ref.A, 1e-10, f"{what} cell {k} A_eff")
                _close(r.correctors[k], want["chi"], 1e-9, f"{what} cell {k} correctors")
                _close(r.strain[k], want["eps"], 1e-9, f"{what} cell {k} strain")
                _close(r.flux[k], want["q"], 1e-9, f"{what} cell {k} flux")
                # the tree route: both remove the mean per component
                _close(r.correctors[k], other.correctors[k], 1e-9, f"{what} cell {k} correctors against the tree route")
                _close(r.flux[k], other.flux[k], 1e-9, f"{what} cell {k} flux against the tree route")
                _close(r.energy[k], other.energy[k], 1e-10, f"{what} cell {k} energy against the tree route")
                _close(r.mean_flux[k], other.mean_flux[k], 1e-10, f"{what} cell {k} mean flux against the tree route")


@pytest.mark.parametrize("dim,kind", CASES)
def test_canonical_loads_reproduce_the_canonical_problem(dim, kind):
    """P = material(coef) e_m: chi_l = chi^m of plan.solve, P_eff[m] = A_H[:, m], energy = C0 - A_H."""
    p = _plan(dim, kind)
    coef, M, _, _, refs = _case(dim, kind)
    P = np.stack([np.transpose(ref.V, (2, 0, 1)) for ref in refs])  # [cell][m][e][:] = V_e e_m
    A, chi = p.solve(coef, M, return_correctors=True)
    r = p.loads(coef, P, M, return_correctors=True)
    for k, ref in enumerate(refs):
        _close(r.P_eff[k], A[k].T, 1e-10, f"{dim}D {kind} cell {k} P_eff = A_H")
        _close(r.correctors[k], chi[k], 1e-9, f"{dim}D {kind} cell {k} correctors")
        _close(r.energy[k], ref.C0 - ref.A, 1e-10, f"{dim}D {kind} cell {k} energy = C0 - A_H")
        _close(r.mean_flux[k], A[k].T, 1e-10, f"{dim}D {kind} cell {k} mean flux = A_H")


# -- second derivatives ----------------------------------------------------------------------------------------------------------------------
def _scale(d2A):
    return np.abs(d2A).max(axis=(1, 2, 3, 4), keepdims=True)


def _close_per_cell(got, want, tol, what):
    err = (np.abs(got - want) / _scale(want)).max()
    print(what, err)
    assert err < tol, (what, err)


def _bitwise_symmetric(d2A):
    return np.array_equal(d2A, np.swapaxes(d2A, 3, 4)) and np.array_equal(d2A, np.swapaxes(d2A, 1, 2))


@functools.lru_cache(maxsize=None)
def _directions(dim, kind):
    """Three shared directions (the coefficient of cell 0, a random stream, the indicator of half the elements) and two per cell."""
    coef = _case(dim, kind)[0]
    rng = np.random.default_rng(7 + 10 * dim + KINDS.index(kind))
    half = np.zeros(coef.shape[1:])
    half[::2] = 1.0
    shared = np.stack([coef[0], rng.standard_normal(coef.shape[1:]), half])
    per_cell = np.stack([coef, rng.standard_normal(coef.shape)], axis=1)
    shared.setflags(write=False)
    per_cell.setflags(write=False)
    return shared, per_cell


@pytest.mark.parametrize("strat", [True, False])
@pytest.mark.parametrize("dim,kind", CASES)
def test_second_derivatives_match_reference(dim, kind, strat):
    p = _plan(dim, kind)
    coef, M, _, _, refs = _case(dim, kind, strat)
    shared, per_cell = _directions(dim, kind)
    r = p.second_sensitivities(coef, M, directions=shared, first=True)
    q = p.second_sensitivities(coef, M, directions=per_cell, per_cell=True, first=True)
    assert r.d2A.shape == (NC, 3, 3, p.t, p.t) and q.d2A.shape == (NC, 2, 2, p.t, p.t) and not r.info.any() and not q.info.any()
    _close_per_cell(r.d2A, np.stack([S2.second_derivatives(c, shared) for c in refs]), TOL2, f"{dim}D {kind} shared directions")
    _close_per_cell(q.d2A, np.stack([S2.second_derivatives(c, per_cell[k]) for k, c in enumerate(refs)]), TOL2, f"{dim}D {kind} per-cell directions")
    assert _bitwise_symmetric(r.d2A) and _bitwise_symmetric(q.d2A)
    assert np.array_equal(r.dA, p.sensitivities(coef, M, directions=shared).dA)  # the first derivatives are those of sensitivities()


# -- invariances, bitwise --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,kind", INVARIANT)
def test_outputs_do_not_depend_on_batch_position_or_on_what_is_asked_for(dim, kind):
    p = _plan(dim, kind)
    coef, M, shared, per_cell, _ = _case(dim, kind)
    full = p.loads(coef, per_cell, M, **FULL)
    perm = [2, 0, 1]
    _assert_equal(p.loads(coef[perm], per_cell[perm], M[perm], **FULL), full, other=perm)
    _assert_equal(p.loads(coef[1:2], per_cell[1:2], M[1:2], **FULL), full, other=slice(1, 2))
    plain, resp = p.loads(coef, per_cell, M), p.loads(coef, per_cell, M, response=True)
    assert plain.energy is None and resp.strain is None and resp.correctors is None
    assert np.array_equal(plain.P_eff, full.P_eff) and np.array_equal(plain.A_eff, full.A_eff)
    for key in ("P_eff", "energy", "mean_flux", "max_flux", "argmax_element"):
        assert np.array_equal(getattr(resp, key), getattr(full, key)), key
    only = p.loads(coef, per_cell, M, return_correctors=True)
    assert only.strain is None and np.array_equal(only.correctors, full.correctors)
    # second derivatives: batch position, with and without dA
    dirs = _directions(dim, kind)[0]
    both = p.second_sensitivities(coef, M, directions=dirs, first=True)
    moved = p.second_sensitivities(coef[perm], M[perm], directions=dirs, first=True)
    assert np.array_equal(moved.d2A, both.d2A[perm]) and np.array_equal(moved.dA, both.dA[perm])
    assert np.array_equal(p.second_sensitivities(coef, M, directions=dirs).d2A, both.d2A)
    assert np.array_equal(p.second_sensitivities(coef, M, directions=dirs[:2]).d2A, both.d2A[:, :2, :2])


@pytest.mark.parametrize("dim,kind", INVARIANT)
def test_a_load_does_not_depend_on_the_loads_beside_it(dim, kind):
    """Row 0 of a two-load call against the one-load call, and load 1 of t alone: a load's sum over the rows of a pivot is formed per
    segment of 32 rows and over the segments in order, whatever the number of loads."""
    p = _plan(dim, kind)
    coef, M, shared, per_cell, _ = _case(dim, kind)
    for P, sl in ((shared, lambda a, b: np.s_[a:b]), (per_cell, lambda a, b: np.s_[:, a:b])):
        two, one = p.loads(coef, P[sl(0, 2)], M, **FULL), p.loads(coef, P[sl(0, 1)], M, **FULL)
        for key in ("P_eff", "mean_flux", "max_flux", "argmax_element", "strain", "flux", "correctors"):
            assert np.array_equal(getattr(two, key)[:, :1], getattr(one, key)), key
        assert np.array_equal(two.energy[:, 0, 0], one.energy[:, 0, 0])
        full, alone = p.loads(coef, P, M, **FULL), p.loads(coef, P[sl(1, 2)], M, **FULL)
        for key in ("P_eff", "mean_flux", "strain", "flux", "correctors"):
            assert np.array_equal(getattr(full, key)[:, 1:2], getattr(alone, key)), key
        assert np.array_equal(full.energy[:, 1, 1], alone.energy[:, 0, 0])


@pytest.mark.parametrize("dim,kind", INVARIANT)
def test_outputs_do_not_depend_on_chunking(dim, kind):
    """HOMMX_RECON_MEM_MB = 1 on a second plan.  A chunk holds, among the rest (the pivot columns of the arena on this route), what
    the host entry streams per cell: the fields [2][t][n_el][t] of a response, and for the second derivatives the t loads [t][n_el][t] of
    one direction.  Twice the cells whose share of that alone fills 1 MB, and one more, cannot run in fewer than three chunks."""
    p, small = _plan(dim, kind), _plan(dim, kind, "front", 1)
    assert small.load_kernel == "mesh_front_subst"
    rng = np.random.default_rng(5)
    for what, per_cell_bytes in (("loads", 8 * 2 * p.t * p.n_el * p.t), ("second", 8 * p.t * p.n_el * p.t)):
        most = (1 << 20) // per_cell_bytes  # no chunk of 1 MB holds more cells than this
        nc = 2 * max(1, most) + 1
        assert -(-nc // max(1, most)) >= 3
        mask = rng.random(p.n_el) < 0.4
        values = np.stack([L.random_coef(kind, dim, 2, rng) for _ in range(nc)])
        M = np.stack([L.random_M(dim, rng) for _ in range(nc)])
        stream, coef = CoefStream.two_phase(mask, values), values[:, mask.astype(int)]
        if what == "loads":
            P = rng.standard_normal((nc, p.t, p.n_el, p.t))
            want = p.loads(stream, P, M, **FULL)
            assert not want.info.any() and np.isfinite(want.correctors).all()
            _assert_equal(small.loads(stream, P, M, **FULL), want)
            shared = L.random_loads(rng, 2, p.n_el, p.t)
            _assert_equal(small.loads(coef, shared, M, response=True), p.loads(coef, shared, M, response=True))
        else:
            dirs = rng.standard_normal((2,) + coef.shape[1:])
            want = p.second_sensitivities(stream, M, directions=dirs, first=True)
            got = small.second_sensitivities(stream, M, directions=dirs, first=True)
            assert not want.info.any() and np.isfinite(want.d2A).all()
            assert np.array_equal(got.d2A, want.d2A) and np.array_equal(got.dA, want.dA) and np.array_equal(got.A_eff, want.A_eff)


@pytest.mark.parametrize("dim,kind", INVARIANT)
@pytest.mark.parametrize("per_cell", [False, True])
def test_device_entries_equal_host_entries(dim, kind, per_cell):
    import torch

    p = _plan(dim, kind)
    coef, M, shared, cell_loads, _ = _case(dim, kind)
    P = cell_loads if per_cell else shared
    want = p.loads(coef, P, M, **FULL)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))  # a copy: the cached case is read only
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    t, nl = p.t, p.t
    out = {"P_eff": empty(NC, nl, t), "A_eff": empty(NC, t, t), "info": empty(NC, dtype=torch.int32), "energy": empty(NC, nl, nl),
           "stats": empty(NC, nl, t + 2), "strain": empty(NC, nl, p.n_el, t), "flux": empty(NC, nl, p.n_el, t),
           "correctors": empty(NC, nl, want.correctors.shape[2])}
    ptr = lambda key: out[key].data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    p.loads_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nl, upload(P), ptr("P_eff"), per_cell, ptr("A_eff"), ptr("info"),
                   ptr("energy"), ptr("stats"), ptr("strain"), ptr("flux"), ptr("correctors"), stream=st)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for key in ("P_eff", "A_eff", "info", "energy", "strain", "flux", "correctors"):
        assert np.array_equal(got[key], getattr(want, key)), key
    assert np.array_equal(got["stats"][:, :, :t], want.mean_flux) and np.array_equal(got["stats"][:, :, t], want.max_flux)
    assert np.array_equal(got["stats"][:, :, t + 1], want.argmax_element)
    # the second derivatives
    dirs = _directions(dim, kind)[1 if per_cell else 0]
    want2 = p.second_sensitivities(coef, M, directions=dirs, per_cell=per_cell, first=True)
    nd = dirs.shape[1 if per_cell else 0]
    d2A = torch.full((NC, nd, nd, t, t), float("nan"), dtype=torch.float64, device=dev)
    dA, A, info = empty(NC, nd, t, t), empty(NC, t, t), empty(NC, dtype=torch.int32)
    p.second_sensitivities_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nd, upload(dirs), d2A.data_ptr(), per_cell,
                                  dA.data_ptr(), A.data_ptr(), info.data_ptr(), stream=st)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d2A.cpu().numpy(), want2.d2A) and np.array_equal(dA.cpu().numpy(), want2.dA)
    assert np.array_equal(A.cpu().numpy(), want2.A_eff) and np.array_equal(info.cpu().numpy(), want2.info)


# -- failure ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,kind", INVARIANT)
def test_bad_cell_is_flagged_and_isolated(dim, kind):
    p = _plan(dim, kind)
    coef, M, shared, _, _ = _case(dim, kind)
    good = p.loads(coef, shared, M, **FULL)
    broken = coef.copy()
    broken[1] = -broken[1]  # a negative coefficient: the first pivot is not positive
    bad = p.loads(broken, shared, M, **FULL)
    assert bad.info[1] != 0 and not bad.info[[0, 2]].any() and not good.info.any()
    assert np.isnan(bad.correctors[1]).all() and np.isnan(bad.energy[1]).all() and np.isnan(bad.mean_flux[1]).all() and np.isnan(bad.flux[1]).all()
    _assert_equal(bad, good, [0, 2], [0, 2])
    dirs = _directions(dim, kind)[0]
    good2 = p.second_sensitivities(coef, M, directions=dirs, first=True)
    bad2 = p.second_sensitivities(broken, M, directions=dirs, first=True)
    assert bad2.info[1] == bad.info[1] and not bad2.info[[0, 2]].any()
    for k in (0, 2):
        assert np.array_equal(bad2.d2A[k], good2.d2A[k]) and np.array_equal(bad2.dA[k], good2.dA[k]) and np.array_equal(bad2.A_eff[k], good2.A_eff[k])


# -- stream order ----------------------------------------------------------------------------------------------------------------------------
DELAY_MS = 100.0  # as tests/test_gpu_stream_order.py derives it
STREAM = {"mesh_front": 24, "mesh_tree": 24}  # the input sets of stream_order_gpu.PLANS: 2D elasticity / 3D Poisson on the two meshes


def _stream_plan(name):
    dim, _, kind, *_ = H.PLANS[name]
    return _plan(dim, kind)


@pytest.mark.parametrize("name", list(STREAM))
def test_loads_device_is_asynchronous_on_its_stream(name):
    p, nc = _stream_plan(name), STREAM[name]
    call = H.call_loads(p, nc, H.inputs(name, nc, 1), H.inputs(name, nc, 2))
    real, _ = H.references(call)
    H.in_flight(call, real, DELAY_MS)


@pytest.mark.parametrize("name", list(STREAM))
def test_second_sensitivities_device_is_asynchronous_on_its_stream(name):
    p, nc = _stream_plan(name), STREAM[name]
    out = {"A_eff": ((nc, p.t, p.t), H.F64), "info": ((nc,), H.I32), "d2A": ((nc, 2, 2, p.t, p.t), H.F64), "dA": ((nc, 2, p.t, p.t), H.F64)}
    call = H.Call("second_sensitivities", p, H.inputs(name, nc, 1), H.inputs(name, nc, 2), ("coef", "M", "dirs"), out,
                  lambda a, st: p.second_sensitivities_device(nc, H._source(a, "sampled"), a["M"], 2, a["dirs"], a["d2A"], False, a["dA"],
                                                              a["A_eff"], a["info"], st))
    real, _ = H.references(call)
    H.in_flight(call, real, DELAY_MS)


# -- end to end ------------------------------------------------------------------------------------------------------------------------------
def _shift_identity(h, P, u0, g, what):
    """P = material(A) E0 with u0 the interpolant of E0 x: solve() with the polarisation and data g = (solve() without it and data g + u0)
    - u0 (the identity of tests/test_gpu_loads.py)."""
    V = h.function_space
    d = h._tdim
    bnd = fem.locate_dofs_geometrical(V, lambda x: np.any([np.isclose(x[k], 0) | np.isclose(x[k], 1) for k in range(d)], axis=0))

    def solve(data):
        gf = fem.Function(V)
        gf.interpolate(data)
        h.set_boundary_conditions(fem.dirichletbc(gf, bnd, V))
        return h.solve().x.array.copy()

    shifted = solve(lambda X: g(X) + u0(X))
    h.set_polarisation(P)
    with_P = solve(g)
    w = fem.Function(V)
    w.interpolate(u0)
    _close(with_P, shifted - w.x.array, 1e-9, what)
    assert not h.cell_info.any()


STEP = 1e-3


def _poisson(scale=1.0):
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.02 * (1.0 + 4.0 * x[0]), lambda x: scale * (0.1 + 0.05 * x[1]))
    return hmm.PoissonHMM(Mm.create_unit_square(4, 4), tp, lambda x: 1.0 + x[0], W.jittered_unit_square(9, 7), 0.01)


def _elasticity(scale=1.0):
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]),  # a fibre along y2
                      lambda x: hmm.Lame(2.0 + x[0], 3.0 + 0 * x[0]), lambda x: hmm.Lame(1.0 + 0 * x[0], scale * (0.5 + 0.2 * x[1])))
    return hmm.LinearElasticityStratifiedHMM(Mm.create_unit_cube(1, 1, 1), tp, lambda x: np.array([0.0, 0.0, -1.0]), W.jittered_unit_cube(3, 4, 3), 0.01,
                                             lambda x: np.array([[1.0, 0.1, 0.05], [0.2, 0.9, 0.2], [-0.1, 0.15, 1.1]]))


def _reference_truncation(h, make, a, b, value):
    """The error of the central difference below on the CPU reference (tests/sens2_ref.py on the same micro mesh, coefficient streams and
    M): its own truncation at this step, relative to the largest exact entry."""
    kind, micro = h._micro_kind(), h._cell_mesh
    cells = np.arange(h._msh.num_cells)
    dirs = h._parameter_directions()[1]
    M = h._stratification(cells)

    def ref_cells(s):
        mask = s._phase_mask().astype(int)
        values = s._coeff.phase_values(s._msh.cell_midpoints()[cells])
        return [S2.on_mesh(micro, kind, values[k][mask], None if M is None else M[k]) for k in cells]

    lo, hi, mid = ref_cells(make(1.0 - STEP)), ref_cells(make(1.0 + STEP)), ref_cells(h)
    fd = np.stack([(S2.first_derivatives(p_, dirs)[b] - S2.first_derivatives(m_, dirs)[b]) / (2.0 * STEP) for p_, m_ in zip(hi, lo)])
    exact = value(h._msh.cell_midpoints().T)[:, None, None] * np.stack([S2.second_derivatives(c, dirs)[a, b] for c in mid])
    return np.abs(fd - exact).max() / np.abs(exact).max()


@pytest.mark.parametrize("make,names,a,b,value,kernel", [
    (_poisson, ("outside", "inside"), 0, 1, lambda c: 0.1 + 0.05 * c[1], "mesh_front"),
    (_elasticity, ("outside.lambda", "outside.mu", "inside.lambda", "inside.mu"), 1, 3, lambda c: 0.5 + 0.2 * c[1], "mesh_front"),
])
def test_solver_classes_end_to_end(make, names, a, b, value, kernel):
    """A solver class on a jittered micro mesh: its plan is the frontal one with the load solve.  The mixed second derivative against
    central differences of ``tensor_derivatives()`` as tests/test_gpu_sens2.py does it: the bound is 10 x the error of the same difference
    on the CPU reference (its truncation at this step) -- the differences, not the kernels, set it --, never below 1e-9, the tolerance of
    d2A itself."""
    h = make()
    r = h.tensor_second_derivatives()
    assert (h._plan.kernel, h._plan.load_kernel) == (kernel, "mesh_front_subst")
    N, t, nd = h._msh.num_cells, h._tensor_size(), len(names)
    assert r.names == names and r.d2A.shape == (N, nd, nd, t, t) and r.dA.shape == (N, nd, t, t) and not r.info.any()
    assert np.array_equal(r.dA, h.tensor_derivatives().dA) and _bitwise_symmetric(r.d2A)
    fd = (make(1.0 + STEP).tensor_derivatives().dA[:, b] - make(1.0 - STEP).tensor_derivatives().dA[:, b]) / (2.0 * STEP)
    exact = value(h._msh.cell_midpoints().T)[:, None, None] * r.d2A[:, a, b]
    err = np.abs(fd - exact).max() / np.abs(exact).max()
    bound = max(10.0 * _reference_truncation(h, make, a, b, value), 1e-9)
    print(names[a], names[b], "mixed second derivative against central differences of tensor_derivatives()", err, "bound", bound)
    assert err < bound
    u = np.random.default_rng(3).standard_normal(h._num_global_dofs)
    xi = h._macro_strains(np.arange(N), u)
    vol = h._msh.cell_volumes() / h._cell_mesh_area
    e = h.energy_second_derivatives(u)
    want = vol[:, None, None] * np.einsum("cm,cabmn,cn->cab", xi, r.d2A, xi)
    assert e.shape == (N, nd, nd) and np.abs(e - want).max() <= 1e-14 * np.abs(want).max()


def test_poisson_hmm_on_a_jittered_micro_mesh():
    E0 = np.array([0.7, -0.4])
    h = _poisson()
    tp = h._coeff
    _shift_identity(h, lambda x, y: [tp(x, y) * E0[0], tp(x, y) * E0[1]], lambda X: E0 @ X[:2], lambda X: 0.3 * X[0] * X[1], "poisson hmm")
    assert (h._plan.kernel, h._plan.load_kernel) == ("mesh_front", "mesh_front_subst")
    _close(h.effective_polarisation, h.effective_tensors @ E0, 1e-10, "P_eff = A_H E0")
    r = h.load_response(cells=[3, 11], fields=True)
    _close(r.mean_flux[:, 0], h.effective_polarisation[[3, 11]], 1e-10, "load_response mean flux")
    total = h.reconstruct(cells=[3, 11], fields=True).flux + r.flux[:, 0]
    assert total.shape == (2, h._cell_mesh.num_cells, 2) and np.isfinite(total).all()
    # solve() does not depend on the flag: a solver whose plan was made without it
    plain = _poisson()
    plain._plan = MicroCellPlan.from_mesh(plain._cell_mesh, "poisson", device=h._plan.device)
    assert plain._plan.load_kernel == "none"
    plain.set_boundary_conditions(h._bcs)
    plain.set_polarisation(h._polarisation)
    assert np.array_equal(plain.solve().x.array, h.solve().x.array) and np.array_equal(plain.effective_tensors, h.effective_tensors)
    with pytest.raises(_lib.HommxLibraryError, match="tree route"):
        plain.load_response(cells=[3])


def test_stratified_elasticity_hmm_on_a_jittered_micro_mesh():
    E = np.array([[0.3, 0.25, -0.1], [0.25, -0.6, 0.2], [-0.1, 0.2, 0.4]])
    lam = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]) + 0.2 * x[1]
    mu = lambda x, y: 0.6 + 0.3 * np.cos(2 * np.pi * y[1]) + 0.1 * x[0]
    tr = np.trace(E)
    P = lambda x, y: [lam(x, y) * tr + 2 * mu(x, y) * E[k, k] for k in range(3)] + [2 * mu(x, y) * E[k, l] for k, l in ((0, 1), (0, 2), (1, 2))]

    def make():
        return hmm.LinearElasticityStratifiedHMM(Mm.create_unit_cube(2, 2, 2), lambda x, y: hmm.Lame(lam(x, y), mu(x, y)),
                                                 lambda x: np.array([0.0, 0.0, -1.0]), W.jittered_unit_cube(3, 4, 3), 0.01,
                                                 lambda x: np.array([[1.0, 0.1, 0.05], [0.2, 0.9, 0.2], [-0.1, 0.15, 1.1]]), quadrature_degree=3)

    h = make()
    _shift_identity(h, P, lambda X: E @ X[:3], lambda X: np.stack([0.1 * X[1] ** 2, 0.2 * X[0] * X[2], 0.05 * X[2]]), "stratified elasticity hmm")
    assert (h._plan.kernel, h._plan.load_kernel) == ("mesh_front", "mesh_front_subst")
    voigt = np.array([E[0, 0], E[1, 1], E[2, 2], 2 * E[0, 1], 2 * E[0, 2], 2 * E[1, 2]])
    _close(h.effective_polarisation, h.effective_tensors @ voigt, 1e-10, "P_eff = C_H : E0")
    r = h.load_response(cells=[0, 17], fields=True)
    _close(r.mean_flux[:, 0], h.effective_polarisation[[0, 17]], 1e-10, "load_response mean flux")
    plain = make()
    plain._plan = MicroCellPlan.from_mesh(plain._cell_mesh, "elasticity", device=h._plan.device)
    plain.set_boundary_conditions(h._bcs)
    plain.set_polarisation(h._polarisation)
    assert np.array_equal(plain.solve().x.array, h.solve().x.array) and np.array_equal(plain.effective_tensors, h.effective_tensors)
