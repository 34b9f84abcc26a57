"""hommx_sensitivity_source[_device] on an MI355X (-m gpu): every (dim, kind, mesh) instantiation of k_sens on the smallest shape of each
route against the NumPy reference (tests/sens_ref.py), the exact identities (symmetry, Euler, sum grad . dir = w : dA), the sampler forms
against the host-formed stream (bitwise), invariance (batch position, chunking, outputs asked for, device against host entry), a failing
cell, the production size, and the solver classes end to end against central differences.

k_sens gathers the correctors from global memory at every size: there is no size-dependent path to straddle."""

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
import sens_ref as S
from hommx_amd import MicroCellPlan, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu

KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")
# name -> (dim, n or None on the jittered mesh of that dimension, kind, route of from_mesh, kernel of the plan's tensor route)
SHAPES = {
    "fused2d_16": (2, 5, "poisson", None, "fused2d"),  # NB = 16
    "fused2d_32": (2, 17, "poisson", None, "fused2d"),  # NB = 32; 578 elements: more than one per thread
    "small_wave_2d": (2, 4, "elasticity", None, "small_wave"),
    "small_wave_3d": (3, 4, "poisson", None, "small_wave"),
    "small_fused": (3, 8, "poisson", None, "small_fused"),
    "multifrontal": (3, 5, "elasticity", None, "multifrontal"),  # 750 elements: no multiple of the 512 threads
    "poisson_matrix_2d": (2, 8, "poisson_matrix", None, None),
    "poisson_matrix_3d": (3, 3, "poisson_matrix", None, None),
    "elasticity_voigt_2d": (2, 4, "elasticity_voigt", None, None),
    "elasticity_voigt_3d": (3, 4, "elasticity_voigt", None, None),
    # the mesh instantiations: the frontal route on the jittered square, the tree route on the jittered cube
    **{f"mesh_front_{k}": (2, None, k, "front", "mesh_front") for k in KINDS},
    **{f"mesh_tree_{k}": (3, None, k, "tree", "mesh_multifrontal") for k in KINDS},
}
NC = 3


@functools.lru_cache(maxsize=None)
def _mesh(dim):
    return W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)


@functools.lru_cache(maxsize=None)
def _plan(name):
    dim, n, kind, route, kernel = SHAPES[name]
    p = MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(_mesh(dim), kind, route=route)
    assert kernel is None or p.kernel == kernel
    return p


def _case(name, strat=True):
    return _cached_case(name, bool(strat))


@functools.lru_cache(maxsize=None)
def _cached_case(name, strat):
    """Three cells of contrast 1e2 with (or without) M, three shared directions -- the coefficient of cell 0, a random stream, the
    indicator of half the elements --, two per-cell directions -- the cell's own coefficient and a random stream --, weights, and the
    reference cells; computed once and shared (read only)."""
    dim, n, kind, _, _ = SHAPES[name]
    p = _plan(name)
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 1000 * strat)
    coef = np.stack([R.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([R.random_M(dim, rng) for _ in range(NC)]) if strat else None
    half = np.zeros(coef.shape[1:])
    half[::2] = 1.0
    shared = np.stack([coef[0], rng.standard_normal(coef.shape[1:]), half])
    per_cell = np.stack([coef, rng.standard_normal(coef.shape)], axis=1)
    w = rng.standard_normal((NC, p.t, p.t))
    refs = [S.structured(kind, dim, n, coef[k], None if M is None else M[k]) if n else S.on_mesh(_mesh(dim), kind, coef[k], None if M is None else M[k])
            for k in range(NC)]
    for a in (coef, shared, per_cell, w) + (() if M is None else (M,)):
        a.setflags(write=False)
    return coef, M, shared, per_cell, w, refs


def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


# -- 1. dA against the reference, symmetry, Euler ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [True, False])
@pytest.mark.parametrize("name", list(SHAPES))
def test_dA_matches_reference(name, strat):
    p = _plan(name)
    coef, M, shared, per_cell, _, refs = _case(name, strat)
    r = p.sensitivities(coef, M, directions=shared)
    q = p.sensitivities(coef, M, directions=per_cell, per_cell=True)
    assert r.dA.shape == (NC, 3, p.t, p.t) and q.dA.shape == (NC, 2, p.t, p.t) and r.grad is None
    assert not r.info.any() and not q.info.any()
    for k, ref in enumerate(refs):
        for d in range(3):
            _close(r.dA[k, d], ref.dA(shared[d]), 1e-9, f"{name} cell {k} shared direction {d}")
        for d in range(2):
            _close(q.dA[k, d], ref.dA(per_cell[k, d]), 1e-9, f"{name} cell {k} per-cell direction {d}")
    for dA in (r.dA, q.dA):
        scale = np.abs(dA).max(axis=(2, 3), keepdims=True)
        assert np.all(np.abs(dA - np.swapaxes(dA, 2, 3)) <= 1e-12 * scale)
    # Euler: the cell's own coefficient as its direction gives the A_eff of plan.solve
    A = p.solve(coef, M)
    _close(q.dA[:, 0], A, 1e-10, f"{name} euler")
    _close(q.A_eff, A, 1e-10, f"{name} A_eff")
    _close(r.dA[0, 0], A[0], 1e-10, f"{name} euler, shared")


# -- 2. the gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradient_matches_reference_and_pairs_with_dA(name):
    """sum grad . dir and w : dA[dir] are sums of the same products |K| w_mn s^m_K . material(dir_K) s^n_K in two orders: they differ by
    a few ulp sqrt(n_el) of the sum of the magnitudes of either side's terms."""
    p = _plan(name)
    coef, M, shared, _, w, refs = _case(name)
    r = p.sensitivities(coef, M, directions=shared, weights=w)
    assert r.grad.shape == coef.shape and not r.info.any()
    for k, ref in enumerate(refs):
        _close(r.grad[k].reshape(p.n_el, -1), ref.grad(w[k], p.n_comp), 1e-9, f"{name} cell {k} grad")
        for d in range(3):
            lhs, rhs = r.grad[k] * shared[d], w[k] * r.dA[k, d]
            err = abs(lhs.sum() - rhs.sum()) / (np.abs(lhs).sum() + np.abs(rhs).sum())
            print(name, k, d, "pairing", err)
            assert err < 1e-12


# -- 3. the sampler forms, bitwise -----------------------------------------------------------------------------------------------------------
def _forms(name, seed):
    """{form: (CoefStream, the element stream the host forms from it)} for NC cells."""
    dim, n, kind, _, _ = SHAPES[name]
    p = _plan(name)
    rng = np.random.default_rng(seed)
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([R.random_coef(kind, dim, 2, rng) for _ in range(NC)])  # two "elements": the two phases of a cell
    forms = {"two_phase": (CoefStream.two_phase(mask, values), values[:, mask.astype(int)])}
    shape = (NC, 2) if kind == "poisson" else (NC, 2, 2)
    params = np.stack([rng.uniform(2.0, 3.0, shape[:-1]), rng.uniform(0.2, 0.8, shape[:-1])], axis=-1)  # a + b g > 0 for |g| <= 1
    wq = np.array([0.2, 0.3, 0.1, 0.4])
    for family in ("affine", "reciprocal") if kind == "poisson" else ("affine",):
        table = rng.uniform(-1.0, 1.0, p.n_el if family == "affine" else (p.n_el, len(wq)))
        forms[family] = (CoefStream.separable(family, table, wq, params), hmm.Separable(family, None, None, None).host_stream(params, table, wq))
    return forms


def _equal(a, b):
    assert np.array_equal(a.dA, b.dA) and np.array_equal(a.A_eff, b.A_eff) and np.array_equal(a.info, b.info)
    assert (a.grad is None) == (b.grad is None) and (a.grad is None or np.array_equal(a.grad, b.grad))


@pytest.mark.parametrize("name", ["fused2d_16", "multifrontal", "mesh_front_poisson", "mesh_tree_elasticity"])
def test_sampler_forms_equal_the_host_formed_stream_bitwise(name):
    p = _plan(name)
    _, M, shared, _, w, _ = _case(name)
    for form, (stream, host_stream) in _forms(name, 11).items():
        want = p.sensitivities(host_stream, M, directions=shared, weights=w)
        assert not want.info.any() and np.isfinite(want.dA).all(), form
        _equal(p.sensitivities(stream, M, directions=shared, weights=w), want)


# -- 4. invariance, bitwise ------------------------------------------------------------------------------------------------------------------
INVARIANT = ["fused2d_32", "multifrontal", "mesh_front_elasticity"]


@pytest.mark.parametrize("name", INVARIANT)
def test_outputs_do_not_depend_on_batch_position_or_on_what_is_asked_for(name):
    p = _plan(name)
    coef, M, shared, per_cell, w, _ = _case(name)
    both = p.sensitivities(coef, M, directions=shared, weights=w)
    perm = [2, 0, 1]
    moved = p.sensitivities(coef[perm], M[perm], directions=shared, weights=w[perm])
    assert np.array_equal(moved.dA, both.dA[perm]) and np.array_equal(moved.grad, both.grad[perm])
    one = p.sensitivities(coef[1:2], M[1:2], directions=per_cell[1:2], per_cell=True)
    assert np.array_equal(one.dA, p.sensitivities(coef, M, directions=per_cell, per_cell=True).dA[1:2])
    assert np.array_equal(p.sensitivities(coef, M, directions=shared).dA, both.dA)
    alone = p.sensitivities(coef, M, weights=w)
    assert alone.dA.shape == (NC, 0, p.t, p.t) and np.array_equal(alone.grad, both.grad)
    assert np.array_equal(p.sensitivities(coef, M, directions=shared[1:2]).dA, both.dA[:, 1:2])


@pytest.mark.parametrize("name", INVARIANT)
@pytest.mark.parametrize("per_cell", [False, True])
def test_device_entry_equals_host_entry(name, per_cell):
    import torch

    p = _plan(name)
    coef, M, shared, cell_dirs, w, _ = _case(name)
    dirs = cell_dirs if per_cell else shared
    want = p.sensitivities(coef, M, directions=dirs, per_cell=per_cell, weights=w)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))  # a copy: the shared case is read only
        return keep[-1].data_ptr()

    nd = dirs.shape[1 if per_cell else 0]
    dA = torch.empty((NC, nd, p.t, p.t), dtype=torch.float64, device=dev)
    grad = torch.empty(coef.shape, dtype=torch.float64, device=dev)
    A = torch.empty((NC, p.t, p.t), dtype=torch.float64, device=dev)
    info = torch.full((NC,), -7, dtype=torch.int32, device=dev)
    p.sensitivities_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nd, upload(dirs), per_cell, dA.data_ptr(), upload(w),
                           grad.data_ptr(), A.data_ptr(), info.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(dA.cpu().numpy(), want.dA) and np.array_equal(grad.cpu().numpy(), want.grad)
    assert np.array_equal(A.cpu().numpy(), want.A_eff) and np.array_equal(info.cpu().numpy(), want.info)


CHUNK_NC = 70  # 3D elasticity, n = 5: 18 KB of correctors and 12 KB of each stream per cell, so 1 MB holds fewer cells than these


def _chunk_case():
    p = MicroCellPlan(3, 5, "elasticity")
    rng = np.random.default_rng(37)
    M = np.stack([R.random_M(3, rng) for _ in range(CHUNK_NC)])
    mask = rng.random(p.n_el) < 0.3
    values = np.stack([R.random_coef("elasticity", 3, 2, rng) for _ in range(CHUNK_NC)])
    shared = rng.standard_normal((2, p.n_el, 2))
    per_cell = rng.standard_normal((CHUNK_NC, 2, p.n_el, 2))
    w = rng.standard_normal((CHUNK_NC, 6, 6))
    a = p.sensitivities(CoefStream.two_phase(mask, values), M, directions=shared, weights=w)  # a sampler form, shared directions
    b = p.sensitivities(values[:, mask.astype(int)], M, directions=per_cell, per_cell=True, weights=w)  # everything per cell
    return {"dA_a": a.dA, "grad_a": a.grad, "A_a": a.A_eff, "dA_b": b.dA, "grad_b": b.grad, "info_b": b.info}


def test_outputs_do_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the batches in chunks of 1 MB."""
    here = _chunk_case()
    assert np.array_equal(here["grad_a"], here["grad_b"]) and not here["info_b"].any()
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, HOMMX_RECON_MEM_MB="1"), timeout=300)
    child = np.load(out)
    for key, want in here.items():
        assert np.array_equal(child[key], want), key


# -- 5. bad cell ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused2d_16", "multifrontal", "mesh_front_poisson"])
def test_bad_cell_is_isolated(name):
    p = _plan(name)
    coef, M, shared, _, w, _ = _case(name)
    good = p.sensitivities(coef, M, directions=shared, weights=w)
    broken = coef.copy()
    broken[1, ::2] = np.nan
    bad = p.sensitivities(broken, M, directions=shared, weights=w)
    assert bad.info[1] != 0 and bad.info[0] == 0 and bad.info[2] == 0 and not good.info.any()
    for k in (0, 2):
        assert np.array_equal(bad.dA[k], good.dA[k]) and np.array_equal(bad.grad[k], good.grad[k]) and np.array_equal(bad.A_eff[k], good.A_eff[k])


# -- 6. production size --------------------------------------------------------------------------------------------------------------------
def test_c5_golden_cells_euler():
    """The three oracle cells of the C5 fixture at 16^3 (24,576 elements, 590 KB of correctors per cell): the Euler identity against the
    committed A_eff, at the tolerance those cells get everywhere else."""
    g = np.load(os.path.join(HERE, "golden", "fullsize_c5_n16_strat.npz"))
    p = MicroCellPlan(3, 16, "elasticity")
    mask = np.unpackbits(g["mask_bits"])[:p.n_el].astype(bool)
    stream = CoefStream.two_phase(mask, g["values"])
    coef = g["values"][:, mask.astype(int)]
    r = p.sensitivities(stream, g["M"], directions=coef[:, None], per_cell=True)
    assert not r.info.any()
    _close(r.dA[:, 0], g["A_eff"], 1e-7, "c5 euler against the golden A_eff")
    _close(r.dA[:, 0], r.A_eff, 1e-7, "c5 euler against the call's own A_eff")


# -- 7. end to end -------------------------------------------------------------------------------------------------------------------------
def test_poisson_hmm_end_to_end():
    """16 x 16 macro cells, 32^2 micro mesh, the wrapped-disc inclusion: d A_H / d inside and the derivative of the macro energy at frozen u
    against central differences with the inside value scaled by 1 +- 1e-5."""
    msh, micro = Mm.create_unit_square(16, 16), Mm.create_unit_square(32, 32)
    inside = lambda x: 0.01 * (1.0 + 9.0 * x[0])

    def solver(scale):
        tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: scale * inside(x), lambda x: 0.1 + 0.0 * x[0])
        return hmm.PoissonHMM(msh, tp, lambda x: 1.0 + x[0], micro, 0.01)

    h = solver(1.0)
    u = h.solve().x.array.copy()
    r = h.tensor_derivatives()
    assert r.names == ("outside", "inside") and r.dA.shape == (msh.num_cells, 2, 2, 2) and not r.info.any()
    _close(r.A_eff, h.effective_tensors, 1e-12, "A_eff of the corrector route against the tensor route")
    step = 1e-5
    hp, hm = solver(1.0 + step), solver(1.0 - step)
    hp.solve(), hm.solve()
    vin = inside(msh.cell_midpoints().T)
    fd = (hp.effective_tensors - hm.effective_tensors) / (2 * step)
    _close(vin[:, None, None] * r.dA[:, 1], fd, 1e-6, "d A_H / d inside against central differences")
    _close(0.1 * r.dA[:, 0] + vin[:, None, None] * r.dA[:, 1], h.effective_tensors, 1e-10, "euler on the two values")
    e = h.energy_derivatives()
    assert e.shape == (msh.num_cells, 2)
    fd_e = (u @ (hp._A @ u) - u @ (hm._A @ u)) / (2 * step)
    err = abs((vin * e[:, 1]).sum() - fd_e) / abs(fd_e)
    print("d (u . K_H u) / d inside against central differences", err)
    assert err < 1e-6
    two = h.tensor_derivatives(cells=[3, 200])
    assert np.array_equal(two.dA, r.dA[[3, 200]])


if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case())
