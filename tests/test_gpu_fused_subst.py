"""Correctors of a fused 2D plan by substitution on the block inverses of the fused kernel itself (-m gpu):
k_poisson2d_fused<NB, true> keeps the factors, k_fused2d_subst substitutes.  Shapes: the smallest at which each mechanism can go wrong --
NB = 16: n = 3 (step 0 and the j = n-2 special case adjacent), 5 (interior steps), 16 (no padding); NB = 32: n = 17 (most padding, the
first real index crosses a tile), 31 (one padding column), 32 (none).  Three cells per case, with and without stratification."""

import functools

import numpy as np
import pytest

from hommx_amd import MicroCellPlan, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream
from oracle import hommx_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [3, 5, 16, 17, 31, 32]
NC = 3


def _centered(cp):
    chi = O.solve_correctors(cp).T  # [t, n_dof]
    return chi - chi.mean(axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _plan(n):
    return MicroCellPlan(2, n, "poisson")


@functools.lru_cache(maxsize=None)
def _case(n, with_M):
    """Inputs, the oracle's mean-free correctors (computed once, shared, left unchanged) and what the plan returns."""
    rng = np.random.default_rng(7000 + 10 * n + with_M)
    coef = np.exp(rng.uniform(np.log(0.1), np.log(5.0), size=(NC, 2 * n * n)))
    M = np.eye(2)[None] + 0.3 * rng.standard_normal((NC, 2, 2)) if with_M else None
    cps = [O.build_cell_problem("poisson", 2, n, coef[c], None if M is None else M[c]) for c in range(NC)]
    ref = np.stack([_centered(cp) for cp in cps])
    ref.setflags(write=False)
    A, corr, info = _plan(n).solve(coef, M, return_info=True, return_correctors=True)
    return coef, M, cps, ref, A, corr, info


CASES = [(n, m) for n in SHAPES for m in (False, True)]


# -- 1. the route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_route_name(n):
    p = _plan(n)
    assert p.kernel == "fused2d" and p.corrector_kernel == "fused2d_subst"


# -- 2. / 3. correctors against the oracle, and through the reference's energy form (tolerances of tests/test_gpu_correctors.py) ---------
@pytest.mark.parametrize("n,with_M", CASES)
def test_correctors_vs_oracle(n, with_M):
    _, _, _, ref, _, corr, info = _case(n, with_M)
    assert np.all(info == 0)
    for c in range(NC):
        err = np.abs(corr[c] - ref[c]).max() / np.abs(ref[c]).max()
        print(f"n={n} M={with_M} cell {c}: corrector error {err:.3e}")
        assert err <= 1e-9
        assert np.abs(corr[c].mean(axis=1)).max() <= 1e-12 * np.abs(ref[c]).max()  # each load case mean-free


@pytest.mark.parametrize("n,with_M", CASES)
def test_energy_form_reproduces_A_eff(n, with_M):
    _, _, cps, _, A, corr, _ = _case(n, with_M)
    for c in range(NC):
        AH = O.effective_tensor(cps[c], corr[c].T, form="energy")
        err = np.abs(AH - A[c]).max() / np.abs(A[c]).max()
        print(f"n={n} M={with_M} cell {c}: energy form error {err:.3e}")
        assert err <= 1e-10


# -- 4. the tensors of the corrector call are those of the tensor call ------------------------------------------------------------------
@pytest.mark.parametrize("n,with_M", CASES)
def test_A_eff_equals_plan_solve(n, with_M):
    coef, M, _, _, A, _, _ = _case(n, with_M)
    A2 = _plan(n).solve(coef, M)
    err = np.abs(A - A2).max() / np.abs(A2).max()
    print(f"n={n} M={with_M}: A_eff of the corrector call against plan.solve {err:.3e}, bitwise {np.array_equal(A, A2)}")
    assert err <= 1e-12


# -- 5. A/B against the plane elimination -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,with_M", CASES)
def test_agrees_with_blocked_route(n, with_M, monkeypatch):
    coef, M, _, ref, _, corr, _ = _case(n, with_M)
    monkeypatch.setenv("HOMMX_FUSED_CORR", "0")  # read when the plan is created
    q = MicroCellPlan(2, n, "poisson")
    assert q.kernel == "fused2d" and q.corrector_kernel == "blocked"
    _, old, info = q.solve(coef, M, return_info=True, return_correctors=True)
    q.close()
    assert np.all(info == 0)
    for c in range(NC):
        s = np.abs(ref[c]).max()
        e_new, e_old, ab = np.abs(corr[c] - ref[c]).max() / s, np.abs(old[c] - ref[c]).max() / s, np.abs(corr[c] - old[c]).max() / s
        print(f"n={n} M={with_M} cell {c}: substitution {e_new:.3e}, plane elimination {e_old:.3e}, A/B {ab:.3e}")
        assert ab <= 2e-9 and e_new <= 1e-9 and e_old <= 1e-9


# -- 6. contrast ---------------------------------------------------------------------------------------------------------------------------
def test_two_phase_contrast_100(monkeypatch):
    n = 32
    y = W.element_barycentres(2, n)
    coef = np.where(W.wrapped_disc(y[:, 0], y[:, 1]), 100.0, 1.0)[None]
    ref = _centered(O.build_cell_problem("poisson", 2, n, coef[0]))
    _, new, info = _plan(n).solve(coef, return_info=True, return_correctors=True)
    assert not info.any()
    monkeypatch.setenv("HOMMX_FUSED_CORR", "0")
    q = MicroCellPlan(2, n, "poisson")
    _, old = q.solve(coef, return_correctors=True)
    q.close()
    s = np.abs(ref).max()
    e_new, e_old = np.abs(new[0] - ref).max() / s, np.abs(old[0] - ref).max() / s
    print(f"contrast 100, n = 32: substitution {e_new:.3e}, plane elimination {e_old:.3e}")
    assert e_new <= max(1e-9, 4.0 * e_old)


# -- 7. position and chunking ----------------------------------------------------------------------------------------------------------------
def _stats(r):
    return np.concatenate([r.mean_strain, r.mean_flux, r.energy[:, None], r.max_flux[:, None], r.argmax_element[:, None]], axis=1)


def test_batch_position_and_chunking(monkeypatch):
    n, nc = 32, 70
    rng = np.random.default_rng(77)
    coef = np.exp(rng.uniform(np.log(0.1), np.log(5.0), size=(nc, 2 * n * n)))
    coef[69] = coef[0]
    M = np.eye(2)[None] + 0.3 * rng.standard_normal((nc, 2, 2))
    M[69] = M[0]
    xi = rng.standard_normal((nc, 2))
    p = _plan(n)
    A, corr, info = p.solve(coef, M, return_info=True, return_correctors=True)
    assert not info.any()
    assert np.array_equal(corr[0], corr[69]) and np.array_equal(A[0], A[69])
    r = p.reconstruct(coef, xi, M)
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")  # read when the plan is created: three cells of factor records and correctors per chunk
    q = MicroCellPlan(2, n, "poisson")
    assert q.corrector_kernel == "fused2d_subst"
    A2, corr2, info2 = q.solve(coef, M, return_info=True, return_correctors=True)
    r2 = q.reconstruct(coef, xi, M)
    q.close()
    assert np.array_equal(corr, corr2) and np.array_equal(A, A2) and np.array_equal(info, info2)
    assert np.array_equal(_stats(r), _stats(r2)) and np.array_equal(r.A_eff, r2.A_eff)


# -- 8. a failing cell stays alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 17])
def test_bad_cell_is_isolated(n):
    rng = np.random.default_rng(80 + n)
    coef = np.exp(rng.uniform(np.log(0.1), np.log(5.0), size=(3, 2 * n * n)))
    p = _plan(n)
    A, corr, info = p.solve(coef, return_info=True, return_correctors=True)
    bad = coef.copy()
    bad[1, n] = np.nan
    Ab, corrb, infob = p.solve(bad, return_info=True, return_correctors=True)
    assert infob[1] != 0 and infob[0] == 0 and infob[2] == 0
    for c in (0, 2):
        assert np.isfinite(corrb[c]).all()
        assert np.array_equal(corrb[c], corr[c]) and np.array_equal(Ab[c], A[c])


# -- 9. sources and solver classes ----------------------------------------------------------------------------------------------------------
def test_sampler_sources_equal_the_host_formed_stream_bitwise():
    n, nc = 17, 4
    p = _plan(n)
    rng = np.random.default_rng(91)
    xi = rng.standard_normal((nc, 2))
    M = np.eye(2)[None] + 0.3 * rng.standard_normal((nc, 2, 2))
    mask = rng.random(p.n_el) < 0.4
    values = np.exp(rng.uniform(np.log(0.1), np.log(5.0), size=(nc, 2)))
    params = np.stack([rng.uniform(2.0, 3.0, nc), rng.uniform(0.2, 0.8, nc)], axis=-1)
    table = rng.uniform(-1.0, 1.0, p.n_el)
    forms = {"two_phase": (CoefStream.two_phase(mask, values), values[:, mask.astype(int)]),
             "affine": (CoefStream.separable("affine", table, None, params), hmm.Separable("affine", None, None, None).host_stream(params, table, None))}
    for form, (stream, host_stream) in forms.items():
        want = p.reconstruct(host_stream, xi, M, fields=True)  # hommx_reconstruct_batch
        got = p.reconstruct(stream, xi, M, fields=True)  # hommx_reconstruct_source
        assert not want.info.any(), form
        assert np.array_equal(_stats(got), _stats(want)) and np.array_equal(got.A_eff, want.A_eff), form
        assert np.array_equal(got.strain, want.strain) and np.array_equal(got.flux, want.flux), form


@pytest.mark.parametrize("strat", [False, True])
def test_solver_class_reconstruct(strat):
    msh, mic = Mm.create_unit_square(4, 4), Mm.create_unit_square(8, 8)
    A = lambda x, y: (1.0 + x[0]) * (2.0 + np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1]))
    if strat:
        Dt = lambda x: np.array([[1.0, -0.5 * np.pi * np.cos(2 * np.pi * x[0])], [0.0, 1.0]])
        h = hmm.PoissonStratifiedHMM(msh, A, lambda x: 1.0, mic, 0.05, Dt)
    else:
        h = hmm.PoissonHMM(msh, A, lambda x: 1.0, mic, 0.05)
    x = h.function_space.tabulate_dof_coordinates()
    r = h.reconstruct(x[:, 0] + 2.0 * x[:, 1] + 0.3 * np.sin(2.0 * x[:, 0]) * np.cos(x[:, 1]))
    assert h._plan.kernel == "fused2d" and h._plan.corrector_kernel == "fused2d_subst"  # the plan the class made for the call
    assert not r.info.any()
    assert np.abs(r.mean_strain - r.xi).max() <= 1e-12 * np.abs(r.xi).max()
    q = np.einsum("ci,cij,cj->c", r.xi, r.A_eff, r.xi)
    assert np.all(np.abs(r.energy - q) <= 1e-10 * np.abs(q))


def test_periodic_hmm_correctors():
    A_y = lambda y: 2.0 + np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1])
    per = hmm.PoissonPeriodicHMM(Mm.create_unit_square(3, 3), A_y, lambda x: 1.0, Mm.create_unit_square(12, 12), 0.05, quadrature_degree=3)
    per.compute_effective_tensor()
    coef = O.sample_coefficient(lambda x, y: A_y(y), np.zeros(2), 2, 12, 3)
    chi = O.solve_correctors(O.build_cell_problem("poisson", 2, 12, coef))
    pm = O.periodic_master_map(2, 12)
    for q, f in enumerate(per.correctors):
        ref = chi[:, q] - chi[:, q].mean()
        assert np.abs(f.x.array - ref[pm]).max() <= 1e-10
