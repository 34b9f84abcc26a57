"""The Python layer on an MI355X (-m gpu): ``MicroCellPlan.reconstruct`` of an array and ``solve_two_phase`` go through the entry
points that take a coefficient source.  The per-form entry points they used to call stay exported and run the same kernels on the same
data, so both pairs agree bit for bit."""

import numpy as np
import pytest

from hommx_amd import MicroCellPlan, _lib

pytestmark = pytest.mark.gpu

NC = 5


def _inputs(p, seed, strat):
    rng = np.random.default_rng(seed)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    coef = 1.0 + rng.random((NC,) + el)
    M = np.eye(p.dim) + 0.2 * rng.random((NC, p.dim, p.dim)) if strat else None
    return rng, coef, M


@pytest.mark.parametrize("strat", [False, True])
@pytest.mark.parametrize("dim,n,kind", [(2, 4, "poisson"), (3, 3, "poisson"), (2, 4, "elasticity"), (3, 3, "elasticity")])
def test_reconstruct_of_an_array_is_hommx_reconstruct_batch(dim, n, kind, strat):
    p = MicroCellPlan(dim, n, kind)
    rng, coef, M = _inputs(p, 10 * dim + n + strat, strat)
    xi = rng.standard_normal((NC, p.t))
    r = p.reconstruct(coef, xi, M, fields=True)
    stats, A, info = np.empty((NC, 2 * p.t + 3)), np.empty((NC, p.t, p.t)), np.full(NC, -1, dtype=np.int32)
    strain, flux = np.empty((NC, p.n_el, p.t)), np.empty((NC, p.n_el, p.t))
    _lib.check(p._lib.hommx_reconstruct_batch(p._h, NC, coef.ctypes.data, None if M is None else M.ctypes.data, xi.ctypes.data, stats.ctypes.data,
                                              strain.ctypes.data, flux.ctypes.data, A.ctypes.data, info.ctypes.data), "hommx_reconstruct_batch")
    assert not info.any() and not r.info.any()
    t = p.t
    for got, want in ((r.mean_strain, stats[:, :t]), (r.mean_flux, stats[:, t:2 * t]), (r.energy, stats[:, 2 * t]), (r.max_flux, stats[:, 2 * t + 1]),
                      (r.argmax_element, stats[:, 2 * t + 2].astype(np.int64)), (r.strain, strain), (r.flux, flux), (r.A_eff, A)):
        assert np.array_equal(got, want)
    assert np.isfinite(r.flux).all() and np.abs(r.flux).max() > 0


@pytest.mark.parametrize("strat", [False, True])
@pytest.mark.parametrize("dim,n,kind", [(2, 4, "poisson"), (3, 3, "poisson"), (2, 4, "elasticity"), (3, 3, "elasticity")])
def test_solve_two_phase_is_hommx_solve_batch_two_phase(dim, n, kind, strat):
    p = MicroCellPlan(dim, n, kind)
    rng, _, M = _inputs(p, 20 * dim + n + strat, strat)
    mask = np.ascontiguousarray(rng.random(p.n_el) < 0.4, dtype=np.uint8)
    values = 1.0 + rng.random((NC, 2) + ((p.n_comp,) if p.n_comp > 1 else ()))
    got, got_info = p.solve_two_phase(mask.astype(bool), values, M, return_info=True)
    A, info = np.empty((NC, p.t, p.t)), np.full(NC, -1, dtype=np.int32)
    _lib.check(p._lib.hommx_solve_batch_two_phase(p._h, NC, mask.ctypes.data, values.ctypes.data, None if M is None else M.ctypes.data,
                                                  A.ctypes.data, info.ctypes.data), "hommx_solve_batch_two_phase")
    assert not info.any() and np.array_equal(got_info, info)
    assert np.array_equal(got, A) and np.isfinite(A).all()
    assert np.array_equal(p.solve_two_phase(mask, values, M), A)  # the same without info, from a uint8 mask
