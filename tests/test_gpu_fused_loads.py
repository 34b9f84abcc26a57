"""The load solve of fused 2D plans by substitution on the factor record (k_fused2d_subst_rhs) on an MI355X (-m gpu),
against the NumPy / SciPy reference (tests/loads_ref.py) and against the plane elimination the same plan takes under HOMMX_FUSED_LOADS=0.

Shapes, the smallest at which the kernel can go wrong: n = 3 (one Horner step, 13 padding columns at NB = 16), 8, 16 (n = NB, no padding),
17 (NB = 32 with the most padding), 20 (more than one element per thread of k_load_stats), 32 (n = NB).  5 cells of distinct coefficients of
contrast 1e2 each.

Tolerances (those of tests/test_gpu_loads.py): 1e-10 for per-cell reductions, 1e-9 for correctors and fields, each relative
to the largest magnitude of the reference array of that cell."""

import contextlib
import functools
import os

import numpy as np
import pytest

import loads_ref as L
from hommx_amd import MicroCellPlan, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu

SHAPES = [3, 8, 16, 17, 20, 32]
NC = 5
FULL = {"fields": True, "return_correctors": True}


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
def _plan(n, fused_loads=True, recon_mb=None):
    """HOMMX_FUSED_LOADS and HOMMX_RECON_MEM_MB are read when the plan is created; the blocked workspace of the yardstick plan by its first
    response call, made here."""
    env = {} if fused_loads else {"HOMMX_FUSED_LOADS": "0"}
    if recon_mb:
        env["HOMMX_RECON_MEM_MB"] = str(recon_mb)
    with _environment(env):
        p = MicroCellPlan(2, n, "poisson")
        rng = np.random.default_rng(0)
        r = p.loads(L.random_coef("poisson", 2, p.n_el, rng)[None], L.random_loads(rng, 1, p.n_el, 2), response=True)
        assert not r.info.any()
    assert p.kernel == "fused2d" and p.corrector_kernel == "fused2d_subst"
    assert p.load_kernel == ("fused2d_subst" if fused_loads else "blocked"), p.load_kernel
    return p


@functools.lru_cache(maxsize=None)
def _case(n, strat=True):
    """NC cells with distinct coefficients (and M), two shared and two per-cell loads, and the reference cells; computed once, read only."""
    rng = np.random.default_rng(n + 100 * strat)
    n_el = 2 * n * n
    coef = np.stack([L.random_coef("poisson", 2, n_el, rng) for _ in range(NC)])
    M = np.stack([L.random_M(2, rng) for _ in range(NC)]) if strat else None
    shared = L.random_loads(rng, 2, n_el, 2)
    per_cell = np.stack([L.random_loads(rng, 2, n_el, 2) for _ in range(NC)])
    refs = [L.structured("poisson", 2, n, coef[k], None if M is None else M[k]) for k in range(NC)]
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


# -- the route -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_load_kernel_names_the_route(n):
    assert _plan(n).load_kernel == "fused2d_subst" and _plan(n, False).load_kernel == "blocked"


def test_load_kernel_of_the_other_plans():
    with _environment({"HOMMX_FUSED_CORR": "0"}):  # no records: the blocked load pass as well
        p = MicroCellPlan(2, 8, "poisson")
    assert (p.corrector_kernel, p.load_kernel) == ("blocked", "blocked")
    p = MicroCellPlan(3, 4, "poisson")
    assert p.kernel == "small_wave" and p.load_kernel == p.corrector_kernel == "blocked"
    p = MicroCellPlan.from_mesh(W.jittered_unit_square(10, 8), "elasticity")
    assert p.kernel == "mesh_front" and p.load_kernel == "none"
    p = MicroCellPlan.from_mesh(W.jittered_unit_square(10, 8), "elasticity", route="tree")
    assert p.load_kernel == p.corrector_kernel == "mesh_multifrontal"


# -- against the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [True, False])
@pytest.mark.parametrize("n", SHAPES)
def test_response_matches_reference(n, strat):
    p = _plan(n)
    coef, M, shared, per_cell, refs = _case(n, strat)
    for nl in (1, 2):
        for P in (shared[:nl], per_cell[:, :nl]):
            what = f"n {n} n_loads {nl} {'per cell' if P.ndim == 4 else 'shared'}"
            r = p.loads(coef, P, M, **FULL)
            assert r.P_eff.shape == (NC, nl, 2) and r.energy.shape == (NC, nl, nl) and r.strain.shape == (NC, nl, p.n_el, 2)
            assert not r.info.any()
            assert np.array_equal(r.energy, np.swapaxes(r.energy, 1, 2))
            for k, ref in enumerate(refs):
                want = ref.solve(P[k] if P.ndim == 4 else P)
                _close(r.P_eff[k], want["P_eff"], 1e-10, f"{what} cell {k} P_eff (Levin)")
                _close(r.mean_flux[k], want["P_eff"], 1e-10, f"{what} cell {k} mean total flux")
                _close(r.energy[k], want["energy"], 1e-10, f"{what} cell {k} energy")
                _close(r.max_flux[k], want["max_flux"], 1e-10, f"{what} cell {k} max flux")
                for l in range(nl):  # the element the device names reaches the reference's maximum
                    assert want["norm"][l, r.argmax_element[k, l]] >= want["max_flux"][l] * (1 - 1e-9)
                _close(r.A_eff[k], ref.A, 1e-10, f"{what} cell {k} A_eff")
                _close(r.correctors[k], want["chi"], 1e-9, f"{what} cell {k} correctors")
                _close(r.strain[k], want["eps"], 1e-9, f"{what} cell {k} strain")
                _close(r.flux[k], want["q"], 1e-9, f"{what} cell {k} flux")


# -- against the plane elimination -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [True, False])
@pytest.mark.parametrize("n", SHAPES)
def test_response_matches_the_plane_elimination(n, strat):
    """The canonical pass is the same code on both plans: bitwise.  The load solve is another algorithm: to the tolerances."""
    coef, M, shared, per_cell, _ = _case(n, strat)
    for P in (shared, per_cell, shared[:1]):
        got, want = _plan(n).loads(coef, P, M, **FULL), _plan(n, False).loads(coef, P, M, **FULL)
        for key in ("A_eff", "P_eff", "info"):
            assert np.array_equal(getattr(got, key), getattr(want, key)), key
        for k in range(NC):
            for key, tol in (("energy", 1e-10), ("mean_flux", 1e-10), ("max_flux", 1e-10), ("correctors", 1e-9), ("strain", 1e-9), ("flux", 1e-9)):
                _close(getattr(got, key)[k], getattr(want, key)[k], tol, f"n {n} cell {k} {key}")


# -- the canonical loads as user loads -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_canonical_loads_reproduce_the_canonical_problem(n):
    """P = material(coef) e_m: chi_l = chi^m, energy = C0 - A_H."""
    p = _plan(n)
    coef, M, _, _, refs = _case(n)
    P = np.stack([np.transpose(ref.V, (2, 0, 1)) for ref in refs])
    A, chi = p.solve(coef, M, return_correctors=True)
    r = p.loads(coef, P, M, return_correctors=True)
    for k, ref in enumerate(refs):
        _close(r.correctors[k], chi[k], 1e-9, f"n {n} cell {k} correctors")
        _close(r.energy[k], ref.C0 - ref.A, 1e-10, f"n {n} cell {k} energy = C0 - A_H")


# -- bitwise invariance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_outputs_do_not_depend_on_batch_position_or_on_what_is_asked_for(n):
    p = _plan(n)
    coef, M, _, per_cell, _ = _case(n)
    full = p.loads(coef, per_cell, M, **FULL)
    perm = [3, 0, 4, 1, 2]
    _assert_equal(p.loads(coef[perm], per_cell[perm], M[perm], **FULL), full, other=perm)
    _assert_equal(p.loads(coef[2:3], per_cell[2:3], M[2:3], **FULL), full, other=slice(2, 3))
    plain, resp = p.loads(coef, per_cell, M), p.loads(coef, per_cell, M, response=True)
    assert plain.energy is None and resp.strain is None and resp.correctors is None
    assert np.array_equal(plain.P_eff, full.P_eff) and np.array_equal(plain.A_eff, full.A_eff)
    for key in ("P_eff", "A_eff", "energy", "mean_flux", "max_flux", "argmax_element"):
        assert np.array_equal(getattr(resp, key), getattr(full, key)), key
    only_chi = p.loads(coef, per_cell, M, return_correctors=True)
    assert np.array_equal(only_chi.correctors, full.correctors)


@pytest.mark.parametrize("n", SHAPES)
def test_row_0_of_a_two_load_call_is_the_one_load_call(n):
    """The load cases sit on separate lanes and never mix; with one load the lanes of the second carry zeros."""
    p = _plan(n)
    coef, M, shared, per_cell, _ = _case(n)
    for P2, P1 in ((per_cell, per_cell[:, :1]), (shared, shared[:1])):
        two, one = p.loads(coef, P2, M, **FULL), p.loads(coef, P1, M, **FULL)
        for key in ("P_eff", "mean_flux", "max_flux", "argmax_element", "correctors", "strain", "flux"):
            assert np.array_equal(getattr(one, key)[:, 0], getattr(two, key)[:, 0]), key
        assert np.array_equal(one.energy[:, 0, 0], two.energy[:, 0, 0])
    swapped = p.loads(coef, shared[::-1], M, **FULL)  # and the same load on the lanes of the other case gives the same corrector
    assert np.array_equal(swapped.correctors[:, 0], two.correctors[:, 1]) and np.array_equal(swapped.correctors[:, 1], two.correctors[:, 0])


@pytest.mark.parametrize("n", SHAPES)
def test_outputs_do_not_depend_on_chunking(n):
    """HOMMX_RECON_MEM_MB = 1 on a second plan.  A chunk of the host entry holds, among the rest, the fields [2][2][n_el][2] of a response per
    cell, so twice the cells whose share of that fills 1 MB, and one more, make three chunks or more (n = 32: 17 cells in chunks of one, the
    factor record counting with the rest); the device-resident route behind the host entry is the same."""
    p, small = _plan(n), _plan(n, True, 1)
    nc = 2 * max(1, (1 << 20) // (8 * 2 * 2 * p.n_el * 2)) + 1
    rng = np.random.default_rng(5)
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([L.random_coef("poisson", 2, 2, rng) for _ in range(nc)])
    M = np.stack([L.random_M(2, rng) for _ in range(nc)])
    shared = L.random_loads(rng, 2, p.n_el, 2)
    per_cell = rng.standard_normal((nc, 2, p.n_el, 2))
    stream, coef = CoefStream.two_phase(mask, values), values[:, mask.astype(int)]
    want = p.loads(stream, per_cell, M, **FULL)
    assert not want.info.any() and np.isfinite(want.correctors).all()
    _assert_equal(small.loads(stream, per_cell, M, **FULL), want)
    _assert_equal(small.loads(coef, shared, M, response=True), p.loads(coef, shared, M, response=True))


@pytest.mark.parametrize("n", SHAPES)
def test_two_phase_stream_equals_its_element_stream_bitwise(n):
    p = _plan(n)
    _, M, shared, _, _ = _case(n)
    rng = np.random.default_rng(11)
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([L.random_coef("poisson", 2, 2, rng) for _ in range(NC)])
    want = p.loads(values[:, mask.astype(int)], shared, M, **FULL)
    assert not want.info.any() and np.isfinite(want.correctors).all()
    _assert_equal(p.loads(CoefStream.two_phase(mask, values), shared, M, **FULL), want)


@pytest.mark.parametrize("per_cell", [False, True])
@pytest.mark.parametrize("n", SHAPES)
def test_device_entry_equals_host_entry(n, per_cell):
    import torch

    p = _plan(n)
    coef, M, shared, cell_loads, _ = _case(n)
    P = cell_loads if per_cell else shared
    want = p.loads(coef, P, M, **FULL)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))  # a copy: the cached case is read only
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    t = nl = 2
    out = {"P_eff": empty(NC, nl, t), "A_eff": empty(NC, t, t), "info": empty(NC, dtype=torch.int32), "energy": empty(NC, nl, nl),
           "stats": empty(NC, nl, t + 2), "strain": empty(NC, nl, p.n_el, t), "flux": empty(NC, nl, p.n_el, t), "correctors": empty(NC, nl, n * n)}
    ptr = lambda key: out[key].data_ptr()
    p.loads_device(NC, CoefStream.sampled(coef).coef_source(upload), upload(M), nl, upload(P), ptr("P_eff"), per_cell, ptr("A_eff"), ptr("info"),
                   ptr("energy"), ptr("stats"), ptr("strain"), ptr("flux"), ptr("correctors"), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for key in ("P_eff", "A_eff", "info", "energy", "strain", "flux", "correctors"):
        assert np.array_equal(got[key], getattr(want, key)), key
    assert np.array_equal(got["stats"][:, :, :t], want.mean_flux) and np.array_equal(got["stats"][:, :, t], want.max_flux)
    assert np.array_equal(got["stats"][:, :, t + 1], want.argmax_element)


# -- magnitude ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_a_power_of_two_in_the_coefficient_is_exact(n):
    """The record is of the coefficient scaled by 2^-esh where the kernel first touches it, the load is scaled with it: with P unchanged a
    coefficient 2^e times as large gives correctors and strains 2^-e times as large and the same fluxes, bit for bit.  A lost esh fails here."""
    p = _plan(n)
    coef, M, shared, per_cell, _ = _case(n)
    for P in (shared, per_cell):
        base = p.loads(coef, P, M, **FULL)
        for e in (40, -40):
            r = p.loads(np.ldexp(coef, e), P, M, **FULL)
            assert not r.info.any()
            assert np.array_equal(r.correctors, np.ldexp(base.correctors, -e)), e
            assert np.array_equal(r.strain, np.ldexp(base.strain, -e)), e
            assert np.array_equal(r.flux, base.flux), e


# -- a failing cell ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_bad_cell_is_flagged_and_isolated(n):
    p = _plan(n)
    coef, M, shared, _, _ = _case(n)
    good = p.loads(coef, shared, M, **FULL)
    broken = coef.copy()
    broken[1] = np.nan
    bad = p.loads(broken, shared, M, **FULL)
    assert bad.info[1] != 0 and not bad.info[[0, 2, 3, 4]].any() and not good.info.any()
    assert np.isnan(bad.correctors[1]).all() and np.isnan(bad.flux[1]).all() and np.isnan(bad.energy[1]).all()
    _assert_equal(bad, good, [0, 2, 3, 4], [0, 2, 3, 4])


# -- end to end ----------------------------------------------------------------------------------------------------------------------------------
def test_poisson_hmm_load_response_on_both_routes():
    E0 = np.array([0.7, -0.4])
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.02 * (1.0 + 4.0 * x[0]), lambda x: 0.1 + 0.05 * x[1])

    def run(env, route):
        with _environment(env):
            h = hmm.PoissonHMM(Mm.create_unit_square(8, 8), tp, lambda x: 1.0 + x[0], Mm.create_unit_square(8, 8), 0.01)
            h.set_polarisation(lambda x, y: [tp(x, y) * E0[0], tp(x, y) * E0[1]])
            u = h.solve().x.array.copy()
            r = h.load_response(fields=True, correctors=True)
        assert h._plan.kernel == "fused2d" and h._plan.load_kernel == route and not h.cell_info.any()
        return u, r

    (u, got), (u0, want) = run({}, "fused2d_subst"), run({"HOMMX_FUSED_LOADS": "0"}, "blocked")
    assert np.array_equal(u, u0)  # the macro solve needs P_eff alone: the canonical pass
    assert np.array_equal(got.P_eff, want.P_eff)
    for key in ("energy", "mean_flux", "max_flux", "correctors", "strain", "flux"):
        _close(getattr(got, key), getattr(want, key), 1e-9, f"hmm {key}")
