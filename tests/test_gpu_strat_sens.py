"""hommx_stratification_sensitivity_source[_device] on an MI355X (-m gpu): every (dim, kind, mesh) instantiation of k_sens_strat on the
smallest shape of each route against the NumPy reference (tests/strat_sens_ref.py), the exact identities (symmetry, pairing with the
weights, zero-homogeneity), M = None against M = I, the laminate closed form, the sampler forms against the host-formed stream (bitwise),
invariance (batch position, outputs asked for, device against host entry, chunking), a failing cell, the production size, and the
stratified solver classes end to end against central differences.

k_sens_strat gathers the correctors from global memory at every size: there is no size-dependent path to straddle."""

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
import strat_sens_ref as S
from hommx_amd import MicroCellPlan, fem, hmm, mesh as Mm, workloads as W
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
    """Three cells of contrast 1e2 with (or without) M, weights, and the reference derivatives; computed once and shared (read only)."""
    dim, n, kind, _, _ = SHAPES[name]
    p = _plan(name)
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 1000 * strat + 77)
    coef = np.stack([R.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([R.random_M(dim, rng) for _ in range(NC)]) if strat else None
    w = rng.standard_normal((NC, p.t, p.t))
    cells = [S.structured(kind, dim, n, coef[k], None if M is None else M[k]) if n else S.on_mesh(_mesh(dim), kind, coef[k], None if M is None else M[k])
             for k in range(NC)]
    dA = np.stack([S.dA_dM(c) for c in cells])
    g = np.stack([S.grad_M(c, w[k]) for k, c in enumerate(cells)])
    for a in (coef, w, dA, g) + (() if M is None else (M,)):
        a.setflags(write=False)
    return coef, M, w, dA, g


def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print(what, err)
    assert err < tol, (what, err)


# -- a, b, c. against the reference, symmetry, pairing, homogeneity ------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [True, False])
@pytest.mark.parametrize("name", list(SHAPES))
def test_matches_reference(name, strat):
    p = _plan(name)
    coef, M, w, dA, g = _case(name, strat)
    r = p.stratification_sensitivities(coef, M, weights=w)
    assert r.dA_dM.shape == (NC, p.dim, p.dim, p.t, p.t) and r.grad_M.shape == (NC, p.dim, p.dim) and not r.info.any()
    for k in range(NC):
        _close(r.dA_dM[k], dA[k], 1e-9, f"{name} cell {k} dA_dM")
        _close(r.grad_M[k], g[k], 1e-9, f"{name} cell {k} grad_M")
    A = p.solve(coef, M)
    _close(r.A_eff, A, 1e-10, f"{name} A_eff")
    assert np.array_equal(r.dA_dM, np.swapaxes(r.dA_dM, 3, 4))
    # pairing: the two sides are sums of the same products in two orders
    for k in range(NC):
        terms = w[k] * r.dA_dM[k]  # [a, b, m, n]
        lhs = terms.sum(axis=(2, 3))
        err = np.abs(lhs - r.grad_M[k]).max() / (np.abs(terms).sum(axis=(2, 3)) + np.abs(r.grad_M[k])).max()
        print(name, k, "pairing", err)
        assert np.all(np.abs(lhs - r.grad_M[k]) <= 1e-12 * (np.abs(terms).sum(axis=(2, 3)) + np.abs(r.grad_M[k])))
    # zero-homogeneity: the corrector error enters to first order
    Mk = np.broadcast_to(np.eye(p.dim), (NC, p.dim, p.dim)) if M is None else M
    hom = np.abs(np.einsum("cab,cabmn->cmn", Mk, r.dA_dM)).max(axis=(1, 2)) / np.abs(r.A_eff).max(axis=(1, 2))
    print(name, "homogeneity", hom.max())
    assert np.all(hom <= 1e-9)


# -- d. M = None is M = I ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_no_M_is_the_identity(name):
    p = _plan(name)
    coef, _, w, _, _ = _case(name, False)
    a = p.stratification_sensitivities(coef, None, weights=w)
    b = p.stratification_sensitivities(coef, np.broadcast_to(np.eye(p.dim), (NC, p.dim, p.dim)).copy(), weights=w)
    _close(b.dA_dM, a.dA_dM, 1e-12, f"{name} dA_dM")
    _close(b.grad_M, a.grad_M, 1e-12, f"{name} grad_M")


# -- e. the laminate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 17])
def test_laminate_closed_form(n):
    p = MicroCellPlan(2, n, "poisson")
    assert p.kernel == "fused2d"
    rng = np.random.default_rng(n)
    a = rng.uniform(1.0, 5.0, (NC, n))
    M = np.stack([R.random_M(2, rng) for _ in range(NC)])
    r = p.stratification_sensitivities(np.stack([S.laminate_coef(n, a[k]) for k in range(NC)]), M)
    assert not r.info.any() and r.grad_M is None
    for k in range(NC):
        A, dA = S.laminate_exact(a[k], M[k])
        errA, err = np.abs(r.A_eff[k] - A).max() / a[k].mean(), np.abs(r.dA_dM[k] - dA).max() / a[k].mean()
        print("laminate", n, k, errA, err)
        assert errA < 1e-10 and err < 1e-10


# -- f. the sampler forms, bitwise ---------------------------------------------------------------------------------------------------------------
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
    assert np.array_equal(a.A_eff, b.A_eff) and np.array_equal(a.info, b.info)
    for x, y in ((a.dA_dM, b.dA_dM), (a.grad_M, b.grad_M)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y))


@pytest.mark.parametrize("name", ["fused2d_16", "multifrontal", "mesh_front_poisson", "mesh_tree_elasticity"])
def test_sampler_forms_equal_the_host_formed_stream_bitwise(name):
    p = _plan(name)
    _, M, w, _, _ = _case(name)
    for form, (stream, host_stream) in _forms(name, 11).items():
        want = p.stratification_sensitivities(host_stream, M, weights=w)
        assert not want.info.any() and np.isfinite(want.dA_dM).all(), form
        _equal(p.stratification_sensitivities(stream, M, weights=w), want)


# -- g. invariance, bitwise --------------------------------------------------------------------------------------------------------------------
INVARIANT = ["fused2d_32", "multifrontal", "mesh_front_elasticity"]


@pytest.mark.parametrize("name", INVARIANT)
def test_outputs_do_not_depend_on_batch_position_or_on_what_is_asked_for(name):
    p = _plan(name)
    coef, M, w, _, _ = _case(name)
    both = p.stratification_sensitivities(coef, M, weights=w)
    perm = [2, 0, 1]
    moved = p.stratification_sensitivities(coef[perm], M[perm], weights=w[perm])
    assert np.array_equal(moved.dA_dM, both.dA_dM[perm]) and np.array_equal(moved.grad_M, both.grad_M[perm])
    one = p.stratification_sensitivities(coef[1:2], M[1:2], weights=w[1:2])
    assert np.array_equal(one.dA_dM, both.dA_dM[1:2]) and np.array_equal(one.grad_M, both.grad_M[1:2])
    full = p.stratification_sensitivities(coef, M)
    assert full.grad_M is None and np.array_equal(full.dA_dM, both.dA_dM)
    alone = p.stratification_sensitivities(coef, M, weights=w, full=False)
    assert alone.dA_dM is None and np.array_equal(alone.grad_M, both.grad_M)


@pytest.mark.parametrize("name", INVARIANT)
def test_device_entry_equals_host_entry(name):
    import torch

    p = _plan(name)
    coef, M, w, _, _ = _case(name)
    want = p.stratification_sensitivities(coef, M, weights=w)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))  # a copy: the shared case is read only
        return keep[-1].data_ptr()

    dA = torch.empty((NC, p.dim, p.dim, p.t, p.t), dtype=torch.float64, device=dev)
    grad = torch.empty((NC, p.dim, p.dim), dtype=torch.float64, device=dev)
    A = torch.empty((NC, p.t, p.t), dtype=torch.float64, device=dev)
    info = torch.full((NC,), -7, dtype=torch.int32, device=dev)
    p.stratification_sensitivities_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), dA.data_ptr(), upload(w), grad.data_ptr(),
                                          A.data_ptr(), info.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(dA.cpu().numpy(), want.dA_dM) and np.array_equal(grad.cpu().numpy(), want.grad_M)
    assert np.array_equal(A.cpu().numpy(), want.A_eff) and np.array_equal(info.cpu().numpy(), want.info)


CHUNK_NC = 70  # 3D elasticity, n = 5: 18 KB of correctors and 12 KB of stream per cell, so 1 MB holds fewer cells than these


def _chunk_case():
    p = MicroCellPlan(3, 5, "elasticity")
    rng = np.random.default_rng(41)
    M = np.stack([R.random_M(3, rng) for _ in range(CHUNK_NC)])
    mask = rng.random(p.n_el) < 0.3
    values = np.stack([R.random_coef("elasticity", 3, 2, rng) for _ in range(CHUNK_NC)])
    w = rng.standard_normal((CHUNK_NC, 6, 6))
    a = p.stratification_sensitivities(CoefStream.two_phase(mask, values), M, weights=w)  # a sampler form
    b = p.stratification_sensitivities(values[:, mask.astype(int)], M, weights=w)  # a sampled stream
    return {"dA_a": a.dA_dM, "grad_a": a.grad_M, "A_a": a.A_eff, "dA_b": b.dA_dM, "grad_b": b.grad_M, "info_b": b.info}


def test_outputs_do_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the batches in chunks of 1 MB."""
    here = _chunk_case()
    assert np.array_equal(here["dA_a"], here["dA_b"]) and np.array_equal(here["grad_a"], here["grad_b"]) and not here["info_b"].any()
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, HOMMX_RECON_MEM_MB="1"), timeout=300)
    child = np.load(out)
    for key, want in here.items():
        assert np.array_equal(child[key], want), key


# -- h. bad cell ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused2d_16", "multifrontal", "mesh_front_poisson"])
def test_bad_cell_is_isolated(name):
    p = _plan(name)
    coef, M, w, _, _ = _case(name)
    good = p.stratification_sensitivities(coef, M, weights=w)
    broken = coef.copy()
    broken[1, ::2] = np.nan
    bad = p.stratification_sensitivities(broken, M, weights=w)
    assert bad.info[1] != 0 and bad.info[0] == 0 and bad.info[2] == 0 and not good.info.any()
    for k in (0, 2):
        assert np.array_equal(bad.dA_dM[k], good.dA_dM[k]) and np.array_equal(bad.grad_M[k], good.grad_M[k])
        assert np.array_equal(bad.A_eff[k], good.A_eff[k])


# -- i. production size --------------------------------------------------------------------------------------------------------------------
def test_c5_golden_cells_homogeneity():
    """The three oracle cells of the C5 fixture at 16^3 (24,576 elements, 590 KB of correctors per cell): zero-homogeneity and the
    committed A_eff, at the tolerance those cells get everywhere else."""
    g = np.load(os.path.join(HERE, "golden", "fullsize_c5_n16_strat.npz"))
    p = MicroCellPlan(3, 16, "elasticity")
    mask = np.unpackbits(g["mask_bits"])[:p.n_el].astype(bool)
    r = p.stratification_sensitivities(CoefStream.two_phase(mask, g["values"]), g["M"])
    assert not r.info.any()
    _close(r.A_eff, g["A_eff"], 1e-7, "c5 A_eff against the golden A_eff")
    hom = np.abs(np.einsum("cab,cabmn->cmn", g["M"], r.dA_dM)).max() / np.abs(r.A_eff).max()
    print("c5 homogeneity", hom, "largest derivative / largest tensor entry", np.abs(r.dA_dM).max() / np.abs(r.A_eff).max())
    assert hom < 1e-7
    assert np.abs(r.dA_dM).max() > 1e-3 * np.abs(r.A_eff).max()  # not vacuous


# -- j, k. end to end ----------------------------------------------------------------------------------------------------------------------
PHI0 = 0.3


def _rotation(phi0):
    def f(x):
        a = phi0 + x[0]
        return [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]

    return f


def _d_rotation(x):
    a = PHI0 + x[0]
    return [[-np.sin(a), -np.cos(a)], [np.cos(a), -np.sin(a)]]


def _end_to_end(solver, msh, subset):
    h = solver(PHI0)
    u = h.solve().x.array.copy()
    r = h.stratification_derivatives(parameters=[_d_rotation])
    t = r.A_eff.shape[1]
    assert r.dA.shape == (msh.num_cells, 1, t, t) and r.dA_dM.shape == (msh.num_cells, 2, 2, t, t) and not r.info.any()
    _close(r.A_eff, h.effective_tensors, 1e-10, "A_eff of the corrector route against the tensor route")
    step = 1e-5
    hp, hm = solver(PHI0 + step), solver(PHI0 - step)
    hp.solve(), hm.solve()
    fd = (hp.effective_tensors - hm.effective_tensors) / (2 * step)
    assert np.abs(fd).max() > 1e-3 * np.abs(r.A_eff).max()  # not vacuous: a disc is nearly isotropic, the derivative is 1 % of the tensor
    _close(r.dA[:, 0], fd, 1e-6, "d A_H / d phi0 against central differences")
    e = h.stratification_energy_derivatives(parameters=[_d_rotation])
    assert e.shape == (msh.num_cells, 1)
    fd_e = (u @ (hp._A @ u) - u @ (hm._A @ u)) / (2 * step)
    err = abs(e.sum() - fd_e) / abs(fd_e)
    print("d (u . K_H u) / d phi0 against central differences", err)
    assert err < 1e-6
    two = h.stratification_derivatives(cells=subset, parameters=[_d_rotation])
    assert np.array_equal(two.dA_dM, r.dA_dM[subset]) and np.array_equal(two.dA, r.dA[subset])


def test_poisson_stratified_hmm_end_to_end():
    """8 x 8 macro cells, 16^2 micro mesh, the wrapped-disc inclusion, Dtheta^T a rotation by phi0 + x0: d A_H / d phi0 and the derivative
    of the macro energy at frozen u against central differences in phi0."""
    msh, micro = Mm.create_unit_square(8, 8), Mm.create_unit_square(16, 16)

    def solver(phi0):
        tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.01 * (1.0 + 9.0 * x[0]), lambda x: 0.1 + 0.0 * x[0])
        return hmm.PoissonStratifiedHMM(msh, tp, lambda x: 1.0 + x[0], micro, 0.01, _rotation(phi0))

    _end_to_end(solver, msh, [3, 100])


def test_elasticity_stratified_hmm_end_to_end():
    """4 x 4 macro cells, 10^2 micro mesh, the same two checks for the rotated two-phase elastic cell."""
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(10, 10)

    def solver(phi0):
        tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: hmm.Lame(10.0 + 5.0 * x[0], 8.0 + 0.0 * x[0]),
                          lambda x: hmm.Lame(1.0 + 0.0 * x[0], 0.5 + 0.0 * x[0]))
        h = hmm.LinearElasticityStratifiedHMM(msh, tp, lambda x: np.array([0.0, -1.0]), micro, 0.01, _rotation(phi0))
        V = h.function_space
        clamp = fem.locate_dofs_topological(V, 1, fem.locate_entities_boundary(msh, 1, lambda x: np.isclose(x[0], 0)))
        h.set_boundary_conditions(fem.dirichletbc(np.zeros(2), clamp, V))
        return h

    _end_to_end(solver, msh, [3, 20])


if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case())
