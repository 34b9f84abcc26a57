"""hommx_second_sensitivity_source[_device] on an MI355X (-m gpu): every (dim, kind, mesh) instantiation of k_sens2_loads / k_sens2 on the
smallest shape of each route against the NumPy / SciPy reference (tests/sens2_ref.py, the energy form; the library sums the direct form),
the exact identities (bitwise symmetry, Euler, concavity, bilinearity), both load routes of the fused 2D plans, the sampler forms against
the host-formed stream (bitwise), invariance (batch position, outputs asked for, device against host entry, chunking), the two ends of
n_dirs (1 and HOMMX_SENS_MAX_DIRS = 8; 0 and 9 refused by the Python layer), a failing cell,
the frontal mesh refusal, the stream-order contract of the device entry, and the solver classes end to end against central differences.

Tolerance: 1e-9 of the cell's max |d2A|, the project's tolerance for correctors and fields (header of tests/test_gpu_loads.py): d2A is
linear in a load corrector whose load is itself formed from the canonical correctors.  This file is the coarse parity check; the accuracy
of d2A is pinned per block against extended precision, at 32 x the float64 yardstick, by tests/test_gpu_accuracy_derived.py.

Both kernels gather the correctors from global memory at every size: there is no size-dependent path to straddle."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child of test_outputs_do_not_depend_on_chunking
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import recon_ref as R
import sens2_ref as S2
from hommx_amd import MicroCellPlan, hmm, mesh as Mm, workloads as W
from hommx_amd._lib import HommxLibraryError
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu

KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")
# name -> (dim, n or None on the jittered cube, kind, kernel of the plan's tensor route): the shapes of tests/test_gpu_sensitivity.py
# without the frontal mesh route, which has no load solve
SHAPES = {
    "fused2d_16": (2, 5, "poisson", "fused2d"),  # NB = 16
    "fused2d_32": (2, 17, "poisson", "fused2d"),  # NB = 32; 578 elements: more than one per thread
    "small_wave_2d": (2, 4, "elasticity", "small_wave"),
    "small_wave_3d": (3, 4, "poisson", "small_wave"),
    "small_fused": (3, 8, "poisson", "small_fused"),
    "multifrontal": (3, 5, "elasticity", "multifrontal"),  # 750 elements: no multiple of the 512 threads
    "poisson_matrix_2d": (2, 8, "poisson_matrix", None),
    "poisson_matrix_3d": (3, 3, "poisson_matrix", None),
    "elasticity_voigt_2d": (2, 4, "elasticity_voigt", None),
    "elasticity_voigt_3d": (3, 4, "elasticity_voigt", None),
    **{f"mesh_tree_{k}": (3, None, k, "mesh_multifrontal") for k in KINDS},
}
NC = 3
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def _mesh():
    return W.jittered_unit_cube(3, 4, 3)


def _new_plan(name):
    dim, n, kind, kernel = SHAPES[name]
    p = MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(_mesh(), kind, route="tree")
    assert kernel is None or p.kernel == kernel
    return p


@functools.lru_cache(maxsize=None)
def _plan(name):
    return _new_plan(name)


def _ref_cell(name, coef, M):
    dim, n, kind, _ = SHAPES[name]
    return S2.structured(kind, dim, n, coef, M) if n else S2.on_mesh(_mesh(), kind, coef, M)


def _case(name, strat=True):
    return _cached_case(name, bool(strat))


@functools.lru_cache(maxsize=None)
def _cached_case(name, strat):
    """Three cells of contrast 1e2 with (or without) M, three shared directions -- the coefficient of cell 0, a random stream, the
    indicator of half the elements --, two per-cell directions -- the cell's own coefficient and a random stream --, and the reference
    d2A of both sets; computed once and shared (read only)."""
    dim, n, kind, _ = SHAPES[name]
    p = _plan(name)
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 1000 * strat)
    coef = np.stack([R.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([R.random_M(dim, rng) for _ in range(NC)]) if strat else None
    half = np.zeros(coef.shape[1:])
    half[::2] = 1.0
    shared = np.stack([coef[0], rng.standard_normal(coef.shape[1:]), half])
    per_cell = np.stack([coef, rng.standard_normal(coef.shape)], axis=1)
    cells = [_ref_cell(name, coef[k], None if M is None else M[k]) for k in range(NC)]
    want_shared = np.stack([S2.second_derivatives(c, shared) for c in cells])
    want_per_cell = np.stack([S2.second_derivatives(c, per_cell[k]) for k, c in enumerate(cells)])
    for a in (coef, shared, per_cell, want_shared, want_per_cell) + (() if M is None else (M,)):
        a.setflags(write=False)
    return coef, M, shared, per_cell, want_shared, want_per_cell


def _scale(d2A):
    """max |d2A| of every cell, broadcastable against d2A[N, a, b, t, t]."""
    return np.abs(d2A).max(axis=(1, 2, 3, 4), keepdims=True)


def _close_per_cell(got, want, tol, what):
    err = (np.abs(got - want) / _scale(want)).max()
    print(what, err)
    assert err < tol, (what, err)


def _bitwise_symmetric(d2A):
    return np.array_equal(d2A, np.swapaxes(d2A, 3, 4)) and np.array_equal(d2A, np.swapaxes(d2A, 1, 2))


# -- 1. d2A against the reference; 2. the identities -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [True, False])
@pytest.mark.parametrize("name", list(SHAPES))
def test_d2A_matches_reference_and_identities(name, strat):
    p = _plan(name)
    coef, M, shared, per_cell, want_shared, want_per_cell = _case(name, strat)
    r = p.second_sensitivities(coef, M, directions=shared, first=True)
    q = p.second_sensitivities(coef, M, directions=per_cell, per_cell=True, first=True)
    assert r.d2A.shape == (NC, 3, 3, p.t, p.t) and q.d2A.shape == (NC, 2, 2, p.t, p.t) and r.dA.shape == (NC, 3, p.t, p.t)
    assert not r.info.any() and not q.info.any()
    _close_per_cell(r.d2A, want_shared, TOL, f"{name} shared directions")
    _close_per_cell(q.d2A, want_per_cell, TOL, f"{name} per-cell directions")
    # the first derivatives of the same call are those of sensitivities(), bit for bit; A_eff is that of solve()
    assert np.array_equal(r.dA, p.sensitivities(coef, M, directions=shared).dA)
    assert np.array_equal(q.dA, p.sensitivities(coef, M, directions=per_cell, per_cell=True).dA)
    A = p.solve(coef, M)
    for got in (r.A_eff, q.A_eff):
        assert np.abs(got - A).max() < 1e-10 * np.abs(A).max()
    for d2A in (r.d2A, q.d2A):
        assert _bitwise_symmetric(d2A)
        # concavity: no diagonal block has a positive eigenvalue
        for a in range(d2A.shape[1]):
            top = np.linalg.eigvalsh(d2A[:, a, a]).max(axis=1)
            print(name, "largest eigenvalue of d2A[a][a] / scale", a, (top / _scale(d2A).ravel()).max())
            assert np.all(top <= TOL * _scale(d2A).ravel())
    # Euler: a block with the cell's own coefficient as one direction vanishes (the random direction keeps the scale non-zero)
    euler = max((np.abs(q.d2A[:, 0]) / _scale(q.d2A)).max(), (np.abs(q.d2A[:, :, 0]) / _scale(q.d2A)).max(),
                np.abs(r.d2A[0, 0]).max() / _scale(r.d2A)[0].max(), np.abs(r.d2A[0, :, 0]).max() / _scale(r.d2A)[0].max())
    print(name, "euler", euler)
    assert euler < TOL and _scale(q.d2A).min() > 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_bilinearity(name):
    p = _plan(name)
    coef, M, shared, _, _, _ = _case(name)
    d = np.stack([shared[1], shared[2], 2.0 * shared[1] - shared[2]])
    r = p.second_sensitivities(coef, M, directions=d)
    want = 4.0 * r.d2A[:, 0, 0] - 4.0 * r.d2A[:, 0, 1] + r.d2A[:, 1, 1]
    err = (np.abs(r.d2A[:, 2, 2] - want) / _scale(r.d2A)[:, 0, 0]).max()
    print(name, "bilinearity", err)
    assert err < TOL and _bitwise_symmetric(r.d2A)


# -- 3. both load routes of the fused plans --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused2d_16", "fused2d_32"])
def test_both_load_routes_of_a_fused_plan(name, monkeypatch):
    """HOMMX_FUSED_LOADS / HOMMX_FUSED_CORR are read when a plan is created: the load solve by substitution on the factor records (the
    default), by one more elimination of the blocked family, and with the canonical correctors from the blocked family as well."""
    coef, M, shared, _, want, _ = _case(name)
    got = {}
    for env, load, corr in ((None, "fused2d_subst", "fused2d_subst"), ("HOMMX_FUSED_LOADS", "blocked", "fused2d_subst"), ("HOMMX_FUSED_CORR", "blocked", "blocked")):
        if env:
            monkeypatch.setenv(env, "0")
        p = _new_plan(name)
        monkeypatch.undo()
        assert (p.load_kernel, p.corrector_kernel) == (load, corr)
        r = p.second_sensitivities(coef, M, directions=shared)
        p.close()
        assert not r.info.any() and _bitwise_symmetric(r.d2A)
        _close_per_cell(r.d2A, want, TOL, f"{name} load route {load}, correctors {corr}")
        got[env] = r.d2A
    _close_per_cell(got["HOMMX_FUSED_LOADS"], got[None], TOL, f"{name} blocked against substitution")
    _close_per_cell(got["HOMMX_FUSED_CORR"], got[None], TOL, f"{name} blocked correctors against substitution")


# -- 4. the sampler forms, bitwise -----------------------------------------------------------------------------------------------------------
def _forms(name, seed):
    """{form: (CoefStream, the element stream the host forms from it)} for NC cells."""
    dim, n, kind, _ = SHAPES[name]
    p = _plan(name)
    rng = np.random.default_rng(seed)
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([R.random_coef(kind, dim, 2, rng) for _ in range(NC)])  # two "elements": the two phases of a cell
    forms = {"two_phase": (CoefStream.two_phase(mask, values), values[:, mask.astype(int)])}
    shape = (NC, 2) if kind == "poisson" else (NC, 2, 2)
    params = np.stack([rng.uniform(2.0, 3.0, shape[:-1]), rng.uniform(0.2, 0.8, shape[:-1])], axis=-1)  # a + b g > 0 for |g| <= 1
    table = rng.uniform(-1.0, 1.0, p.n_el)
    forms["affine"] = (CoefStream.separable("affine", table, None, params), hmm.Separable("affine", None, None, None).host_stream(params, table, None))
    return forms


def _equal(a, b):
    assert np.array_equal(a.d2A, b.d2A) and np.array_equal(a.A_eff, b.A_eff) and np.array_equal(a.info, b.info)
    assert (a.dA is None) == (b.dA is None) and (a.dA is None or np.array_equal(a.dA, b.dA))


@pytest.mark.parametrize("name", ["fused2d_16", "multifrontal", "mesh_tree_elasticity"])
def test_sampler_forms_equal_the_host_formed_stream_bitwise(name):
    p = _plan(name)
    _, M, shared, _, _, _ = _case(name)
    for form, (stream, host_stream) in _forms(name, 11).items():
        want = p.second_sensitivities(host_stream, M, directions=shared[1:], first=True)
        assert not want.info.any() and np.isfinite(want.d2A).all() and np.abs(want.d2A).max() > 0, form
        _equal(p.second_sensitivities(stream, M, directions=shared[1:], first=True), want)


# -- 5. invariance, bitwise ------------------------------------------------------------------------------------------------------------------
INVARIANT = ["fused2d_32", "multifrontal", "mesh_tree_elasticity"]


@pytest.mark.parametrize("name", INVARIANT)
def test_outputs_do_not_depend_on_batch_position_or_on_what_is_asked_for(name):
    p = _plan(name)
    coef, M, shared, per_cell, _, _ = _case(name)
    both = p.second_sensitivities(coef, M, directions=shared, first=True)
    perm = [2, 0, 1]
    moved = p.second_sensitivities(coef[perm], M[perm], directions=shared, first=True)
    assert np.array_equal(moved.d2A, both.d2A[perm]) and np.array_equal(moved.dA, both.dA[perm])
    alone = p.second_sensitivities(coef[1:2], M[1:2], directions=per_cell[1:2], per_cell=True)
    assert alone.dA is None
    assert np.array_equal(alone.d2A, p.second_sensitivities(coef, M, directions=per_cell, per_cell=True, first=True).d2A[1:2])
    assert np.array_equal(p.second_sensitivities(coef, M, directions=shared).d2A, both.d2A)  # without dA
    # fewer directions: the blocks they share do not change
    assert np.array_equal(p.second_sensitivities(coef, M, directions=shared[:2]).d2A, both.d2A[:, :2, :2])


@pytest.mark.parametrize("name", INVARIANT)
@pytest.mark.parametrize("per_cell", [False, True])
def test_device_entry_equals_host_entry(name, per_cell):
    import torch

    p = _plan(name)
    coef, M, shared, cell_dirs, _, _ = _case(name)
    dirs = cell_dirs if per_cell else shared
    want = p.second_sensitivities(coef, M, directions=dirs, per_cell=per_cell, first=True)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))  # a copy: the shared case is read only
        return keep[-1].data_ptr()

    nd = dirs.shape[1 if per_cell else 0]
    d2A = torch.full((NC, nd, nd, p.t, p.t), float("nan"), dtype=torch.float64, device=dev)
    dA = torch.empty((NC, nd, p.t, p.t), dtype=torch.float64, device=dev)
    A = torch.empty((NC, p.t, p.t), dtype=torch.float64, device=dev)
    info = torch.full((NC,), -7, dtype=torch.int32, device=dev)
    p.second_sensitivities_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nd, upload(dirs), d2A.data_ptr(), per_cell,
                                  dA.data_ptr(), A.data_ptr(), info.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d2A.cpu().numpy(), want.d2A) and np.array_equal(dA.cpu().numpy(), want.dA)
    assert np.array_equal(A.cpu().numpy(), want.A_eff) and np.array_equal(info.cpu().numpy(), want.info)


# -- 5b. the two ends of n_dirs ----------------------------------------------------------------------------------------------------------------
MAX_DIRS = 8  # HOMMX_SENS_MAX_DIRS


@functools.lru_cache(maxsize=None)
def _eight(name):
    """Eight shared directions whose first three are the case's, eight per-cell directions whose first two are the case's, and the
    reference d2A of both; computed once (read only)."""
    coef, M, shared, per_cell, _, _ = _case(name)
    rng = np.random.default_rng(77 + sorted(SHAPES).index(name))
    shared8 = np.concatenate([shared, rng.standard_normal((MAX_DIRS - 3,) + shared.shape[1:])])
    per_cell8 = np.concatenate([per_cell, rng.standard_normal((NC, MAX_DIRS - 2) + per_cell.shape[2:])], axis=1)
    cells = [_ref_cell(name, coef[k], M[k]) for k in range(NC)]
    want_shared = np.stack([S2.second_derivatives(c, shared8) for c in cells])
    want_per_cell = np.stack([S2.second_derivatives(c, per_cell8[k]) for k, c in enumerate(cells)])
    for a in (shared8, per_cell8, want_shared, want_per_cell):
        a.setflags(write=False)
    return shared8, per_cell8, want_shared, want_per_cell


@pytest.mark.parametrize("name", INVARIANT)
@pytest.mark.parametrize("per_cell", [False, True])
def test_one_and_eight_directions(name, per_cell):
    """n_dirs = HOMMX_SENS_MAX_DIRS: all 36 blocks a <= b (and their mirror images) against the reference; the blocks of the first three
    directions and of the first one are the bits of the calls with three directions and with one.  Per cell, the directions of a chunk
    start at c0 * n_dirs * (elements * components)."""
    p = _plan(name)
    coef, M = _case(name)[:2]
    shared8, per_cell8, want_shared, want_per_cell = _eight(name)
    dirs, want = (per_cell8, want_per_cell) if per_cell else (shared8, want_shared)
    first = lambda n: dirs[:, :n] if per_cell else dirs[:n]  # noqa: E731
    r8 = p.second_sensitivities(coef, M, directions=dirs, per_cell=per_cell, first=True)
    assert r8.d2A.shape == (NC, MAX_DIRS, MAX_DIRS, p.t, p.t) and r8.dA.shape == (NC, MAX_DIRS, p.t, p.t) and not r8.info.any()
    assert _bitwise_symmetric(r8.d2A)
    _close_per_cell(r8.d2A, want, TOL, f"{name} eight {'per-cell' if per_cell else 'shared'} directions")
    assert np.array_equal(r8.dA, p.sensitivities(coef, M, directions=dirs, per_cell=per_cell).dA)
    for n in (3, 1):
        r = p.second_sensitivities(coef, M, directions=first(n), per_cell=per_cell, first=True)
        assert r.d2A.shape == (NC, n, n, p.t, p.t) and not r.info.any()
        assert np.array_equal(r.d2A, r8.d2A[:, :n, :n]) and np.array_equal(r.dA, r8.dA[:, :n]) and np.array_equal(r.A_eff, r8.A_eff), n


@pytest.mark.parametrize("per_cell", [False, True])
def test_python_layer_refuses_zero_and_nine_directions(per_cell, monkeypatch):
    """Before any device call: the plan's host-call path is never entered.  (The C side: test_abi.py's argument test.)"""
    p = _plan("fused2d_16")
    coef, M = _case("fused2d_16")[:2]

    def never(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(p, "_host_call", never)
    for n in (0, MAX_DIRS + 1):
        dirs = np.ones(((NC,) if per_cell else ()) + (n, p.n_el))
        with pytest.raises(ValueError, match="n_dirs must be 1 .. 8"):
            p.second_sensitivities(coef, M, directions=dirs, per_cell=per_cell)
    monkeypatch.undo()
    assert not p.second_sensitivities(coef, M, directions=np.ones((1, p.n_el))).info.any()  # the refusals left the plan usable


# Cells per chunk of 1 MB (recon_chunk of api.hip; per cell: two blocks of t correctors, t n_el t doubles of loads, on the fused plan the
# factor record and the refinement scratch, and the host entry's staging blocks):
#   fused2d_32            n = 17: 207,600 B (157 KB of it the factor record) and up to 19 KB of staging -> 4 cells: 12 cells run as 4 + 4 + 4
#                         (the device blocks do not depend on n_dirs: one direction's loads at a time; with eight per-cell directions
#                         the staging of the host entry grows to 46 KB -- 37 KB of directions --: 254 KB a cell, still 4 cells)
#   multifrontal          3D elasticity n = 5: 2 x 18 KB + 216 KB of loads and up to 36 KB of staging -> 3 or 4 cells: 10 cells run in 3 or 4 chunks
#   mesh_tree_elasticity  216 elements, 36 nodes: 2 x 5 KB + 62 KB and up to 10 KB of staging -> 12 to 14 cells: 30 cells run in 3 chunks
#   elasticity_8          3D elasticity n = 8 (not in SHAPES): 2 x 74 KB + 885 KB = 1,032,192 B before any staging -> ONE cell per chunk: 3 cells, 3 chunks
CHUNKED = {"fused2d_32": 12, "multifrontal": 10, "mesh_tree_elasticity": 30, "elasticity_8": 3}


def _chunk_case():
    out = {}
    for name, nc in CHUNKED.items():
        p = MicroCellPlan(3, 8, "elasticity") if name == "elasticity_8" else _new_plan(name)
        kind, dim = p.kind, p.dim
        rng = np.random.default_rng(41 + nc)
        M = np.stack([R.random_M(dim, rng) for _ in range(nc)])
        mask = rng.random(p.n_el) < 0.3
        values = np.stack([R.random_coef(kind, dim, 2, rng) for _ in range(nc)])
        el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
        shared = rng.standard_normal((2,) + el)
        per_cell = rng.standard_normal((nc, 2) + el)
        a = p.second_sensitivities(CoefStream.two_phase(mask, values), M, directions=shared, first=True)  # a sampler form, shared directions
        b = p.second_sensitivities(values[:, mask.astype(int)], M, directions=per_cell, per_cell=True)  # everything per cell
        out.update({f"{name}.d2A_a": a.d2A, f"{name}.dA_a": a.dA, f"{name}.A_a": a.A_eff, f"{name}.d2A_b": b.d2A, f"{name}.info_b": b.info})
        if name == "fused2d_32":  # HOMMX_SENS_MAX_DIRS per-cell directions: the directions of a chunk start at c0 * 8 * n_el
            eight = rng.standard_normal((nc, 8) + el)
            c = p.second_sensitivities(values[:, mask.astype(int)], M, directions=eight, per_cell=True, first=True)
            out.update({f"{name}.d2A_c": c.d2A, f"{name}.dA_c": c.dA, f"{name}.info_c": c.info})
        p.close()
    return out


def test_outputs_do_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the batches in chunks of 1 MB (CHUNKED)."""
    here = _chunk_case()
    assert not any(v.any() for k, v in here.items() if k.endswith(("info_b", "info_c")))
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, HOMMX_RECON_MEM_MB="1"), timeout=300)
    child = np.load(out)
    for key, want in here.items():
        assert np.array_equal(child[key], want), key


# -- 6. a failing cell -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused2d_16", "multifrontal", "mesh_tree_poisson"])
def test_bad_cell_is_isolated(name):
    p = _plan(name)
    coef, M, shared, _, _, _ = _case(name)
    good = p.second_sensitivities(coef, M, directions=shared, first=True)
    broken = coef.copy()
    broken[1] = -broken[1]  # a negative coefficient: the first pivot is not positive
    bad = p.second_sensitivities(broken, M, directions=shared, first=True)
    assert bad.info[1] != 0 and bad.info[0] == 0 and bad.info[2] == 0 and not good.info.any()
    for k in (0, 2):
        assert np.array_equal(bad.d2A[k], good.d2A[k]) and np.array_equal(bad.dA[k], good.dA[k]) and np.array_equal(bad.A_eff[k], good.A_eff[k])


# -- 7. the frontal mesh plan ----------------------------------------------------------------------------------------------------------------
def test_frontal_mesh_plan_is_refused_and_the_tree_route_works():
    msh = W.jittered_unit_square(9, 7)
    rng = np.random.default_rng(5)
    coef = np.stack([R.random_coef("poisson", 2, msh.num_cells, rng) for _ in range(NC)])
    M = np.stack([R.random_M(2, rng) for _ in range(NC)])
    dirs = rng.standard_normal((2, msh.num_cells))
    front = MicroCellPlan.from_mesh(msh, "poisson", route="front")
    assert front.kernel == "mesh_front" and front.load_kernel == "none"
    with pytest.raises(HommxLibraryError, match="tree route"):
        front.second_sensitivities(coef, M, directions=dirs)
    assert np.isfinite(front.sensitivities(coef, M, directions=dirs).dA).all()  # the refusal left the plan usable
    front.close()
    tree = MicroCellPlan.from_mesh(msh, "poisson", route="tree")
    r = tree.second_sensitivities(coef, M, directions=dirs)
    tree.close()
    want = np.stack([S2.second_derivatives(S2.on_mesh(msh, "poisson", coef[k], M[k]), dirs) for k in range(NC)])
    assert not r.info.any()
    _close_per_cell(r.d2A, want, TOL, "tree route on the jittered square")


# -- 8. stream order -------------------------------------------------------------------------------------------------------------------------
DELAY_MS = 100.0  # as tests/test_gpu_stream_order.py derives it
STREAM_CELLS = {"fused2d_32": 24, "small_wave": 24, "multifrontal": 40, "mesh_tree": 40}  # its CELLS: 40 cells fork onto the side streams


@pytest.mark.parametrize("name", list(STREAM_CELLS))
def test_device_entry_is_asynchronous_on_its_stream(name):
    """The in-flight protocol of tests/stream_order_gpu.py: the call on a non-blocking stream behind inputs still held back, bitwise
    against the synchronised null-stream call.  Two shared directions, dA asked for."""
    import stream_order_gpu as H

    p, nc = H.plan(name), STREAM_CELLS[name]
    out = {"A_eff": ((nc, p.t, p.t), H.F64), "info": ((nc,), H.I32), "d2A": ((nc, 2, 2, p.t, p.t), H.F64), "dA": ((nc, 2, p.t, p.t), H.F64)}
    call = H.Call("second_sensitivities", p, H.inputs(name, nc, 1), H.inputs(name, nc, 2), ("coef", "M", "dirs"), out,
                  lambda a, st: p.second_sensitivities_device(nc, H._source(a, "sampled"), a["M"], 2, a["dirs"], a["d2A"], False, a["dA"],
                                                              a["A_eff"], a["info"], st))
    real, _ = H.references(call)
    H.in_flight(call, real, DELAY_MS)


# -- 9. end to end ---------------------------------------------------------------------------------------------------------------------------
STEP = 1e-3


def _poisson(scale=1.0):
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.01 * (1.0 + 9.0 * x[0]), lambda x: scale * (0.1 + 0.05 * x[1]))
    return hmm.PoissonHMM(Mm.create_unit_square(4, 4), tp, lambda x: 1.0 + x[0], Mm.create_unit_square(8, 8), 0.01)


def _elasticity(scale=1.0):
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: hmm.Lame(2.0 + x[0], 3.0 + 0 * x[0]),
                      lambda x: hmm.Lame(1.0 + 0 * x[0], scale * (0.5 + 0.2 * x[1])))
    return hmm.LinearElasticityHMM(Mm.create_unit_square(4, 4), tp, lambda x: np.zeros(2), Mm.create_unit_square(4, 4), 0.01)


@pytest.mark.parametrize("make,names,a,b,value,bound", [
    (_poisson, ("outside", "inside"), 0, 1, lambda c: 0.1 + 0.05 * c[1], 4.0e-6),
    (_elasticity, ("outside.lambda", "outside.mu", "inside.lambda", "inside.mu"), 1, 3, lambda c: 0.5 + 0.2 * c[1], 4.6e-7),
])
def test_solver_classes_end_to_end(make, names, a, b, value, bound):
    """4 x 4 macro cells, the wrapped-disc inclusion on an 8^2 (Poisson) / 4^2 (elasticity) micro mesh.  The mixed entry d2A[a][b] -- outside
    value (Poisson) / outside mu (elasticity) against the inside one -- against central differences of ``tensor_derivatives()`` of solvers
    built with that outside value scaled by 1 +- 1e-3.  On the CPU reference (the same solver classes on stub plans that answer from
    tests/sens2_ref.py) that difference is off by 4.0e-7 (Poisson) and 4.5e-8 (elasticity) of the largest entry at this step -- its own
    truncation: 4.0e-9 / 4.5e-10 at 1e-4 --; the bound is 10 x that: the differences, not the kernels, set it."""
    h = make()
    r = h.tensor_second_derivatives()
    N, t, nd = h._msh.num_cells, h._tensor_size(), len(names)
    assert r.names == names and r.d2A.shape == (N, nd, nd, t, t) and r.dA.shape == (N, nd, t, t) and not r.info.any()
    assert np.array_equal(r.dA, h.tensor_derivatives().dA) and _bitwise_symmetric(r.d2A)
    fd = (make(1.0 + STEP).tensor_derivatives().dA[:, b] - make(1.0 - STEP).tensor_derivatives().dA[:, b]) / (2.0 * STEP)
    exact = value(h._msh.cell_midpoints().T)[:, None, None] * r.d2A[:, a, b]
    err = np.abs(fd - exact).max() / np.abs(exact).max()
    print(names[a], names[b], "mixed second derivative against central differences of tensor_derivatives()", err)
    assert err < bound
    # the energy form of the solver class against the host contraction
    u = np.random.default_rng(3).standard_normal(h._num_global_dofs)
    cells = np.arange(N)
    xi = h._macro_strains(cells, u)
    vol = h._msh.cell_volumes() / h._cell_mesh_area
    e = h.energy_second_derivatives(u)
    want = vol[:, None, None] * np.einsum("cm,cabmn,cn->cab", xi, r.d2A, xi)
    assert e.shape == (N, nd, nd) and np.abs(e - want).max() <= 1e-14 * np.abs(want).max()
    two = h.tensor_second_derivatives(cells=[3, 11])
    assert np.array_equal(two.d2A, r.d2A[[3, 11]])


if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case())
