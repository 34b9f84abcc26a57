"""Reconstruction from a coefficient source and per-region statistics on the CPU: the argument checks of hommx_reconstruct_source[_device]
(they run before any device is touched), the hommx_coef_source a CoefStream fills, and BaseHMM.reconstruct on oracle-backed stub plans --
a TwoPhase coefficient reaches the plan as its CoefStream, a stand-in without the sampler methods still gets element means, the region
means are the region sums over the region volume (no GPU needed)."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib, hmm, mesh
from hommx_amd.batch import CoefStream, Reconstruction, region_labels
from test_reconstruct_host import ReconOraclePlan


# -- C ABI argument checks ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _fake_plan(kind):
    """Plan-shaped memory whose descriptor names `kind`: the checks under test read nothing else of it."""
    fake = ctypes.create_string_buffer(4096)
    ctypes.memmove(fake, ctypes.byref(_lib.PlanDesc(2, 8, kind, 0, 0)), ctypes.sizeof(_lib.PlanDesc))
    return fake


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_reconstruct_source_device if device_entry else lib.hommx_reconstruct_source
    tail = (None,) if device_entry else ()

    def call(plan, src, n_regions=0, region=None, region_stats=None, n_cells=1):
        rc = fn(plan, n_cells, src, None, p, n_regions, region, p, region_stats, None, None, None, None, *tail)
        return rc, lib.hommx_last_error().decode()

    sampled = _lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p)
    two = _lib.CoefSource(form=_lib.COEF_TWO_PHASE, mask=p, values=p)
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan = ctypes.addressof(fake)
    assert lib.hommx_plan_kind(plan) == _lib.KIND_POISSON_SCALAR
    rc, msg = call(None, ctypes.byref(sampled))
    assert rc == -1 and "null plan" in msg
    assert call(None, ctypes.byref(sampled), n_cells=0)[0] == -1  # null plan, even when empty
    rc, msg = call(plan, None)
    assert rc == -1 and "null source" in msg
    rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=7, coef=p)))
    assert rc == -1 and "unknown coefficient form 7" in msg
    for src in (_lib.CoefSource(form=_lib.COEF_SAMPLED), _lib.CoefSource(form=_lib.COEF_TWO_PHASE, mask=p),
                _lib.CoefSource(form=_lib.COEF_SEPARABLE, family=_lib.SAMPLER_AFFINE, table=p)):
        rc, msg = call(plan, ctypes.byref(src))
        assert rc == -1 and "null" in msg
    rc, msg = call(plan, ctypes.byref(sampled), 9, p, p)
    assert rc == -1 and "n_regions" in msg
    for nr, region, rstats in ((3, p, None), (3, None, p), (0, p, None), (0, None, p), (2, None, p), (3, None, p)):
        rc, msg = call(plan, ctypes.byref(sampled), nr, region, rstats)  # (2, None, p): only a two-phase source lends its mask
        assert rc == -1 and "region and region_stats" in msg, (nr, region, rstats)
    rc, msg = call(plan, ctypes.byref(two), 3, None, p)  # ... and only for two regions
    assert rc == -1 and "region and region_stats" in msg
    # the separable form: the restrictions and texts of hommx_solve_batch_separable
    rec = _lib.CoefSource(form=_lib.COEF_SEPARABLE, family=_lib.SAMPLER_RECIPROCAL, n_q=3, table=p, weights=p, params=p)
    elast = _fake_plan(_lib.KIND_ELASTICITY_ISO)
    assert lib.hommx_plan_kind(ctypes.addressof(elast)) == _lib.KIND_ELASTICITY_ISO
    rc, msg = call(ctypes.addressof(elast), ctypes.byref(rec))
    assert rc == -1 and "isotropic elasticity kind takes the affine sampler only" in msg
    rc, msg = call(ctypes.addressof(_fake_plan(_lib.KIND_POISSON_MATRIX)), ctypes.byref(rec))
    assert rc == -1 and "separable samplers are defined for the scalar Poisson and the isotropic elasticity kinds" in msg
    rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=_lib.COEF_SEPARABLE, family=5, table=p, params=p)))
    assert rc == -1 and "unknown sampler family 5" in msg
    rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=_lib.COEF_SEPARABLE, family=_lib.SAMPLER_RECIPROCAL, n_q=0, table=p, weights=p, params=p)))
    assert rc == -1 and "reciprocal sampler needs n_q >= 1 and weights" in msg
    # a well-formed source passes on to the shared checks of the reconstruct entry points
    rc = fn(plan, 1, ctypes.byref(two), None, None, 2, None, p, p, None, None, None, None, *tail)
    assert rc == -1 and "null coef / xi / stats" in lib.hommx_last_error().decode()
    assert call(plan, ctypes.byref(two), n_cells=-1)[0] == -1


# -- the Python forms --------------------------------------------------------------------------------------------------------------
def test_coef_source_spells_the_three_forms():
    coef, mask, values = np.ones((3, 8)), np.arange(8) % 2 == 0, np.ones((3, 2))
    table, w, params = np.ones((8, 4)), np.full(4, 0.25), np.ones((3, 2))
    s = CoefStream.sampled(coef)
    src = s.coef_source()
    assert (src.form, src.coef, src.mask, src.table) == (_lib.COEF_SAMPLED, s.per_cell.ctypes.data, None, None)
    s = CoefStream.two_phase(mask, values)
    src = s.coef_source()
    assert (src.form, src.mask, src.values, src.coef) == (_lib.COEF_TWO_PHASE, s.shared[0].ctypes.data, s.per_cell.ctypes.data, None)
    assert s.shared[0].dtype == np.uint8
    s = CoefStream.separable("reciprocal", table, w, params)
    src = s.coef_source()
    assert (src.form, src.family, src.n_q) == (_lib.COEF_SEPARABLE, _lib.SAMPLER_RECIPROCAL, 4)
    assert (src.table, src.weights, src.params) == (s.shared[1].ctypes.data, s.shared[2].ctypes.data, s.per_cell.ctypes.data)
    src = CoefStream.separable("affine", table[:, 0], w, params).coef_source(address=lambda a: 4096)  # e.g. an upload
    assert (src.family, src.n_q, src.table, src.weights, src.params) == (_lib.SAMPLER_AFFINE, 1, 4096, None, 4096)


def test_region_labels():
    lab, n = region_labels(np.array([0, 2, -1, 300, 255, 1]), 6)
    assert lab.dtype == np.uint8 and list(lab) == [0, 2, 255, 255, 255, 1] and n == 3
    lab, n = region_labels(np.array([True, False]), 2)
    assert list(lab) == [1, 0] and n == 2
    assert region_labels(np.array([0, 9, 1]), 3)[1] == 2  # a label from 8 up is in no region
    assert region_labels(np.array([0, 1, 1]), 3, 4)[1] == 4
    for bad, kw in ((np.zeros(3), {}), (np.zeros(4, int), {}), (np.full(3, 9), {}), (np.zeros(3, int), {"n_regions": 9})):
        with pytest.raises(ValueError):
            region_labels(bad, 3, **kw)


# -- solver classes on oracle-backed stub plans -------------------------------------------------------------------------------------------
class SourceOraclePlan(ReconOraclePlan):
    """A stand-in with the sampler method of the two-phase form, so the solver classes hand it that form as the CoefStream; it
    expands the stream as the library does, and forms the region rows of the library's layout from the reference's fields."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.seen = []

    def solve_two_phase(self, mask, values, M=None, return_info=False):
        return self.solve(values[:, np.asarray(mask).astype(int)], M, return_info)

    def reconstruct(self, coef, xi, M=None, fields=False, regions=None, n_regions=0):
        self.seen.append(coef)
        if isinstance(coef, CoefStream):
            assert coef.method == "solve_two_phase"
            coef = coef.per_cell[:, coef.shared[0].astype(int)]
        r = super().reconstruct(coef, xi, M, fields=True)
        if regions is None:
            return r if fields else Reconstruction.from_stats(r.xi, _stats(r), r.A_eff, r.info)
        n_el, t = r.strain.shape[1:]
        rs = np.zeros((len(xi), n_regions, 2 * t + 4))
        rs[:, :, -2:] = -1.0
        for k in range(n_regions):
            el = np.nonzero(regions == k)[0]
            if el.size == 0:
                continue
            s, q = r.strain[:, el], r.flux[:, el]
            nrm = np.linalg.norm(q, axis=2)
            rs[:, k] = np.concatenate([np.full((len(xi), 1), el.size / n_el), s.sum(axis=1) / n_el, q.sum(axis=1) / n_el,
                                       np.einsum("cet,cet->c", s, q)[:, None] / n_el, nrm.max(axis=1)[:, None],
                                       el[np.argmax(nrm, axis=1)][:, None]], axis=1)
        return Reconstruction.from_stats(r.xi, _stats(r), r.A_eff, r.info, r.strain if fields else None, r.flux if fields else None, region_stats=rs)


def _stats(r):
    return np.concatenate([r.mean_strain, r.mean_flux, r.energy[:, None], r.max_flux[:, None], r.argmax_element[:, None]], axis=1)


def two_phase_solver(plan_cls, nx=3, n=4):
    A = hmm.TwoPhase(lambda y: (y[0] > 0.25) & (y[0] < 0.75) & (y[1] < 0.5), lambda x: 5.0 + 2.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: 1.0, mesh.create_unit_square(n, n), 0.01)
    h._plan = plan_cls(2, n, "poisson")
    return h


def _macro_field(h):
    x = h.function_space.tabulate_dof_coordinates()[:, :2]
    return np.sin(2.0 * x[:, 0]) + x[:, 1] ** 2


def test_two_phase_reaches_the_plan_as_its_stream(monkeypatch):
    h = two_phase_solver(SourceOraclePlan)
    u = _macro_field(h)

    def no_means(self, cells):
        raise AssertionError("a device-sampled coefficient must not be sampled on the host")

    monkeypatch.setattr(hmm.BaseHMM, "_element_means", no_means)
    r = h.reconstruct(u)
    (seen,) = h._plan.seen
    assert isinstance(seen, CoefStream) and seen.method == "solve_two_phase"
    assert seen.per_cell.shape == (h._msh.num_cells, 2) and seen.shared[0].shape == (32,)
    monkeypatch.undo()
    # a stand-in without the sampler method gets the same coefficient as element means, and answers the same numbers
    g = two_phase_solver(ReconOraclePlan)
    got = []
    g._plan.reconstruct = lambda coef, *a, _f=g._plan.reconstruct, **kw: (got.append(coef), _f(coef, *a, **kw))[1]
    e = g.reconstruct(u)
    assert isinstance(got[0], np.ndarray) and got[0].shape == (h._msh.num_cells, 32)
    for name in ("xi", "mean_strain", "mean_flux", "energy", "max_flux", "argmax_element"):
        assert np.array_equal(getattr(r, name), getattr(e, name)), name
    assert r.region_volume is None and e.region_mean_flux is None


def test_chunks_are_sized_by_the_outputs_for_sampler_forms():
    h = two_phase_solver(SourceOraclePlan)
    u = _macro_field(h)
    h.reconstruct(u, chunk_cells=5)
    assert [len(s) for s in h._plan.seen] == [5, 5, 5, 3]
    full, parts = h.reconstruct(u, regions=True), h.reconstruct(u, regions=True, chunk_cells=7)
    for name in ("energy", "region_volume", "region_mean_flux", "region_max_flux", "region_argmax_element"):
        assert np.array_equal(getattr(full, name), getattr(parts, name)), name


def test_regions_true_needs_a_two_phase_coefficient():
    g = hmm.PoissonHMM(mesh.create_unit_square(2, 2), lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]), lambda x: 1.0,
                       mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
    g._plan = SourceOraclePlan(2, 4, "poisson")
    with pytest.raises(ValueError, match="TwoPhase"):
        g.reconstruct(np.zeros(g._num_global_dofs), regions=True)


@pytest.mark.parametrize("form", ["true", "array", "callable"])
def test_region_means_are_sums_over_volume(form):
    h = two_phase_solver(SourceOraclePlan)
    u = _macro_field(h)
    mid = h._cell_mesh.cell_midpoints()[:, :2].T
    inside = np.asarray(h._coeff.indicator(mid), dtype=bool)
    if form == "true":
        lab, regions, R = inside.astype(int), True, 2
    else:  # three regions of which region 1 is empty, and a few elements in none
        fn = lambda y: np.where(y[1] > 0.75, 255, np.where(y[0] < 0.5, 0, 2))
        lab, regions, R = fn(mid), (fn if form == "callable" else fn(mid)), 3
    r = h.reconstruct(u, regions=regions, fields=True)
    n_el, nc = len(lab), h._msh.num_cells
    assert r.region_volume.shape == (nc, R) and r.region_mean_flux.shape == (nc, R, 2) and r.region_argmax_element.shape == (nc, R)
    for k in range(R):
        el = np.nonzero(lab == k)[0]
        if el.size == 0:
            assert np.all(r.region_volume[:, k] == 0) and np.isnan(r.region_mean_strain[:, k]).all() and np.isnan(r.region_mean_flux[:, k]).all()
            assert np.all(r.region_energy[:, k] == 0) and np.all(r.region_max_flux[:, k] == -1) and np.all(r.region_argmax_element[:, k] == -1)
            continue
        assert np.allclose(r.region_volume[:, k], el.size / n_el, rtol=1e-14)
        assert np.allclose(r.region_mean_flux[:, k], r.flux[:, el].mean(axis=1), rtol=1e-12, atol=1e-14)  # equal volumes: the plain mean
        assert np.allclose(r.region_mean_strain[:, k], r.strain[:, el].mean(axis=1), rtol=1e-12, atol=1e-14)
        nrm = np.linalg.norm(r.flux[:, el], axis=2)
        assert np.array_equal(r.region_max_flux[:, k], nrm.max(axis=1))
        assert np.array_equal(r.region_argmax_element[:, k], el[np.argmax(nrm, axis=1)])
    if form == "true":  # the two phases cover the cell
        assert np.allclose(np.einsum("cr,crt->ct", r.region_volume, r.region_mean_flux), r.mean_flux, rtol=1e-12, atol=1e-14)
        assert np.allclose(r.region_energy.sum(axis=1), r.energy, rtol=1e-12)
        assert np.array_equal(r.region_max_flux.max(axis=1), r.max_flux)
