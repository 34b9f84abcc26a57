"""hommx_reconstruct_source[_device] on an MI355X (-m gpu): the sampler forms against hommx_reconstruct_batch on the host-formed stream
(bitwise), the per-region statistics against the NumPy reference (tests/recon_ref.py) and their exact identities, invariance (fields,
chunking, the REGIONS instantiation against the plain one), a failing cell, and the solver classes end to end.  One shape per route."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child of test_region_stats_do_not_depend_on_chunking
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import recon_ref as R
from hommx_amd import MicroCellPlan, fem, hmm, mesh as Mm, workloads as W
from hommx_amd.batch import CoefStream

pytestmark = pytest.mark.gpu

# name -> (dim, n or None on the jittered 6 x 6 mesh, kind, route of from_mesh, kernel of the plan's tensor route)
SHAPES = {
    "fused2d": (2, 8, "poisson", None, "fused2d"),  # the corrector workspace is created lazily
    "small_wave_2d": (2, 6, "elasticity", None, "small_wave"),
    "small_wave_3d": (3, 4, "poisson", None, "small_wave"),
    "small_fused": (3, 8, "poisson", None, "small_fused"),
    "multifrontal": (3, 5, "elasticity", None, "multifrontal"),  # b = 75; 750 elements: no multiple of the 512 threads
    "mesh_front": (2, None, "poisson", "front", "mesh_front"),
    "mesh_tree": (2, None, "poisson", "tree", "mesh_multifrontal"),
    "poisson_matrix": (2, 8, "poisson_matrix", None, None),
    "elasticity_voigt": (2, 6, "elasticity_voigt", None, None),
}
NC = 4


@functools.lru_cache(maxsize=None)
def _mesh():
    return W.jittered_unit_square(6, 6)


@functools.lru_cache(maxsize=None)
def _plan(name):
    dim, n, kind, route, kernel = SHAPES[name]
    p = MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(_mesh(), kind, route=route)
    assert kernel is None or p.kernel == kernel
    return p


def _t(kind, dim):
    return dim if kind.startswith("poisson") else dim * (dim + 1) // 2


def _stats(r):
    return np.concatenate([r.mean_strain, r.mean_flux, r.energy[:, None], r.max_flux[:, None], r.argmax_element[:, None]], axis=1)


def _region_rows(r):
    """The numbers the library returned, as it returned them: [volume | max | argmax] (the means are quotients formed in Python)."""
    return np.stack([r.region_volume, r.region_max_flux, r.region_argmax_element, r.region_energy], axis=2)


def _region_sums(r):
    """[volume | sum strain | sum flux | energy | max | argmax] per region: the means times the volume (0 for an empty region)."""
    v = r.region_volume[:, :, None]
    z = lambda a: np.where(v > 0, a * v, 0.0)
    return np.concatenate([v, z(r.region_mean_strain), z(r.region_mean_flux), r.region_energy[:, :, None], r.region_max_flux[:, :, None],
                           r.region_argmax_element[:, :, None]], axis=2)


def _inputs(name, seed, nc=NC):
    """xi, M and one coefficient per form for `nc` cells: {form: (CoefStream, the element stream the host forms from it)}."""
    dim, n, kind, _, _ = SHAPES[name]
    p = _plan(name)
    rng = np.random.default_rng(seed)
    xi = rng.standard_normal((nc, _t(kind, dim)))
    M = np.stack([R.random_M(dim, rng) for _ in range(nc)])
    mask = rng.random(p.n_el) < 0.4
    values = np.stack([R.random_coef(kind, dim, 2, rng) for _ in range(nc)])  # two "elements": the two phases of a cell
    forms = {"two_phase": (CoefStream.two_phase(mask, values), values[:, mask.astype(int)])}
    if kind in ("poisson", "elasticity"):
        shape = (nc, 2) if kind == "poisson" else (nc, 2, 2)
        params = np.stack([rng.uniform(2.0, 3.0, shape[:-1]), rng.uniform(0.2, 0.8, shape[:-1])], axis=-1)  # a + b g > 0 for |g| <= 1
        w = np.array([0.2, 0.3, 0.1, 0.4])
        for family in ("affine", "reciprocal") if kind == "poisson" else ("affine",):
            table = rng.uniform(-1.0, 1.0, p.n_el if family == "affine" else (p.n_el, len(w)))
            forms[family] = (CoefStream.separable(family, table, w, params), hmm.Separable(family, None, None, None).host_stream(params, table, w))
    return xi, M, forms


def _equal(a, b, fields=True):
    assert np.array_equal(_stats(a), _stats(b))
    assert np.array_equal(a.A_eff, b.A_eff) and np.array_equal(a.info, b.info)
    if fields:
        assert np.array_equal(a.strain, b.strain) and np.array_equal(a.flux, b.flux)


# -- 1. form equivalence, bitwise --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_sampler_forms_equal_the_host_formed_stream_bitwise(name):
    import torch

    p = _plan(name)
    xi, M, forms = _inputs(name, 11)
    dev = torch.device("cuda", p.device)
    for form, (stream, host_stream) in forms.items():
        want = p.reconstruct(host_stream, xi, M, fields=True)  # hommx_reconstruct_batch
        assert not want.info.any(), form
        got = p.reconstruct(stream, xi, M, fields=True)  # hommx_reconstruct_source
        _equal(got, want)
        _equal(p.reconstruct(stream, xi, None), p.reconstruct(host_stream, xi, None), fields=False)
        # the device entry
        keep = []

        def upload(a):
            keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
            return keep[-1].data_ptr()

        t = p.t
        st = torch.empty((NC, 2 * t + 3), dtype=torch.float64, device=dev)
        s = torch.empty((NC, p.n_el, t), dtype=torch.float64, device=dev)
        q = torch.empty_like(s)
        A = torch.empty((NC, t, t), dtype=torch.float64, device=dev)
        info = torch.full((NC,), -7, dtype=torch.int32, device=dev)
        p.reconstruct_source_device(NC, stream.coef_source(upload), upload(M), upload(xi), st.data_ptr(), strain_ptr=s.data_ptr(),
                                    flux_ptr=q.data_ptr(), A_ptr=A.data_ptr(), info_ptr=info.data_ptr(),
                                    stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert np.array_equal(st.cpu().numpy(), _stats(want)), form
        assert np.array_equal(s.cpu().numpy(), want.strain) and np.array_equal(q.cpu().numpy(), want.flux)
        assert np.array_equal(A.cpu().numpy(), want.A_eff) and np.array_equal(info.cpu().numpy(), want.info)


# -- 2. regions against the reference ------------------------------------------------------------------------------------------------------
def _labels(n_el):
    """Regions 0 and 1 interleaved element by element, region 2 a handful of elements (fewer than a wave), some elements in no region;
    with n_regions = 4 region 3 is empty."""
    lab = np.arange(n_el) % 2
    lab[np.arange(n_el) % 7 == 3] = 255
    lab[[5, 17, 40, n_el // 2, n_el - 1]] = 2
    return lab


@functools.lru_cache(maxsize=None)
def _sampled_case(name):
    """A sampled random stream with its reference fields, computed once and shared (read only)."""
    dim, n, kind, _, _ = SHAPES[name]
    p = _plan(name)
    rng = np.random.default_rng(23)
    coef = np.stack([R.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)])
    M = np.stack([R.random_M(dim, rng) for _ in range(NC)])
    xi = rng.standard_normal((NC, _t(kind, dim)))
    refs = [R.structured(kind, dim, n, coef[k], M[k], xi[k]) if n else R.on_mesh(_mesh(), kind, coef[k], M[k], xi[k]) for k in range(NC)]
    vol = np.full(p.n_el, 1.0 / p.n_el) if n else _mesh().cell_volumes()
    for a in (coef, M, xi, vol):
        a.setflags(write=False)
    return coef, M, xi, refs, vol


def _scales(xi, coef):
    """Per cell: |xi| (strain sums), |xi| max coef (flux sums, max) and |xi|^2 max coef (energy)."""
    nx = np.linalg.norm(xi, axis=1)
    mc = np.abs(coef.reshape(len(xi), -1)).max(axis=1)
    return nx, nx * mc, nx * nx * mc


@pytest.mark.parametrize("name", list(SHAPES))
def test_region_stats_match_reference(name):
    p = _plan(name)
    coef, M, xi, refs, vol = _sampled_case(name)
    t = p.t
    lab = _labels(p.n_el)
    r = p.reconstruct(coef, xi, M, regions=lab, n_regions=4)
    assert not r.info.any()
    got = _region_sums(r)
    s_scale, q_scale, e_scale = _scales(xi, coef)
    for k, ref in enumerate(refs):
        nrm = np.sqrt((ref["q"] ** 2 * np.where(np.arange(t) >= p.dim, 2.0, 1.0)).sum(axis=1))  # Frobenius: shear entries twice
        for reg in range(3):
            el = np.nonzero(lab == reg)[0]
            row = got[k, reg]
            print(name, k, reg, abs(row[0] - vol[el].sum()), np.abs(row[1:1 + t] - vol[el] @ ref["s"][el]).max() / s_scale[k],
                  np.abs(row[1 + t:1 + 2 * t] - vol[el] @ ref["q"][el]).max() / q_scale[k],
                  abs(row[1 + 2 * t] - vol[el] @ (ref["s"][el] * ref["q"][el]).sum(axis=1)) / e_scale[k], abs(row[2 + 2 * t] - nrm[el].max()) / q_scale[k])
            assert abs(row[0] - vol[el].sum()) < 1e-12
            assert np.abs(row[1:1 + t] - vol[el] @ ref["s"][el]).max() < 1e-10 * s_scale[k]
            assert np.abs(row[1 + t:1 + 2 * t] - vol[el] @ ref["q"][el]).max() < 1e-10 * q_scale[k]
            assert abs(row[1 + 2 * t] - vol[el] @ (ref["s"][el] * ref["q"][el]).sum(axis=1)) < 1e-10 * e_scale[k]
            assert abs(row[2 + 2 * t] - nrm[el].max()) < 1e-10 * q_scale[k]
            assert int(row[3 + 2 * t]) == el[np.argmax(nrm[el])]
        assert np.array_equal(got[k, 3], np.r_[np.zeros(2 * t + 2), -1.0, -1.0])  # the empty region, exactly
        assert np.isnan(r.region_mean_flux[k, 3]).all() and np.isnan(r.region_mean_strain[k, 3]).all()


# -- 3. identities with labels that cover the cell, 4. the REGIONS instantiation against the plain one --------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_region_identities_and_invariance(name):
    p = _plan(name)
    coef, M, xi, _, _ = _sampled_case(name)
    t = p.t
    lab = (np.arange(p.n_el) * 5 // 3) % 3
    plain = p.reconstruct(coef, xi, M)
    r = p.reconstruct(coef, xi, M, regions=lab)
    assert r.region_volume.shape == (NC, 3)
    s_scale, q_scale, e_scale = _scales(xi, coef)
    scale = np.concatenate([np.repeat(s_scale[:, None], t, 1), np.repeat(q_scale[:, None], t, 1), e_scale[:, None]], axis=1)
    assert np.abs(r.region_volume.sum(axis=1) - 1.0).max() < 1e-12
    sums = _region_sums(r)[:, :, 1:2 * t + 2].sum(axis=1)
    print(name, (np.abs(sums - _stats(r)[:, :2 * t + 1]) / scale).max(), (np.abs(_stats(r) - _stats(plain))[:, :2 * t + 1] / scale).max())
    assert np.all(np.abs(sums - _stats(r)[:, :2 * t + 1]) < 1e-12 * scale)
    assert np.array_equal(r.region_max_flux.max(axis=1), r.max_flux)  # bitwise: the same instructions per element in every pass
    top = np.argmax(r.region_max_flux, axis=1)
    assert np.array_equal(r.region_argmax_element[np.arange(NC), top], r.argmax_element)
    assert np.array_equal(lab[r.region_argmax_element], np.broadcast_to(np.arange(3), (NC, 3)))
    # whole-cell statistics of the REGIONS instantiation against the plain one: the same reduction order
    assert np.all(np.abs(_stats(r) - _stats(plain))[:, :2 * t + 1] < 1e-12 * scale)
    assert np.all(np.abs(r.max_flux - plain.max_flux) < 1e-12 * q_scale) and np.array_equal(r.argmax_element, plain.argmax_element)
    # fields on and off
    f = p.reconstruct(coef, xi, M, regions=lab, fields=True)
    assert np.array_equal(_region_rows(f), _region_rows(r)) and np.array_equal(f.region_mean_flux, r.region_mean_flux)
    assert np.array_equal(f.region_mean_strain, r.region_mean_strain) and np.array_equal(_stats(f), _stats(r))
    g = p.reconstruct(coef, xi, M, fields=True)
    assert np.array_equal(f.strain, g.strain) and np.array_equal(f.flux, g.flux)


CHUNK_NC = 70  # 3D elasticity, n = 5: 18 KB of correctors per cell, so 1 MB holds 58 cells without fields and 11 with


def _chunk_case():
    p = MicroCellPlan(3, 5, "elasticity")
    rng = np.random.default_rng(37)
    xi = rng.standard_normal((CHUNK_NC, 6))
    M = np.stack([R.random_M(3, rng) for _ in range(CHUNK_NC)])
    mask = rng.random(p.n_el) < 0.3
    values = np.stack([R.random_coef("elasticity", 3, 2, rng) for _ in range(CHUNK_NC)])
    out = {}
    for fields in (False, True):
        r = p.reconstruct(CoefStream.two_phase(mask, values), xi, M, fields=fields, regions=True)  # the mask as the labels
        out[f"stats{int(fields)}"], out[f"rows{int(fields)}"] = _stats(r), _region_sums(r)
    lab = np.where(np.arange(p.n_el) % 5 == 0, 255, np.arange(p.n_el) % 3)
    r = p.reconstruct(values[:, mask.astype(int)], xi, M, regions=lab)
    out["stats_s"], out["rows_s"] = _stats(r), _region_sums(r)
    return out, mask


def test_region_stats_do_not_depend_on_chunking(tmp_path):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh child process runs the batch in chunks of 1 MB of correctors."""
    here, mask = _chunk_case()
    assert np.array_equal(here["rows0"], here["rows1"]) and np.array_equal(here["stats0"], here["stats1"])
    assert np.all(here["rows0"][:, 1, 0] > 0) and abs(here["rows0"][0, 1, 0] - mask.mean()) < 1e-12  # region 1 is phase 1
    out = str(tmp_path / "chunked.npz")
    env = dict(os.environ, HOMMX_RECON_MEM_MB="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, timeout=300)
    child = np.load(out)
    for key, want in here.items():
        assert np.array_equal(child[key], want), key


# -- 5. bad cell ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused2d", "multifrontal", "mesh_front"])
def test_bad_cell_is_isolated(name):
    p = _plan(name)
    xi, M, forms = _inputs(name, 43, nc=6)
    stream, _ = forms["two_phase"]
    lab = _labels(p.n_el)
    good = p.reconstruct(stream, xi, M, regions=lab, n_regions=4)
    values = stream.per_cell.copy()
    values[2, 1, ...] = np.nan
    bad = p.reconstruct(CoefStream.two_phase(stream.shared[0], values), xi, M, regions=lab, n_regions=4)
    assert bad.info[2] != 0 and not np.delete(bad.info, 2).any() and not good.info.any()
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(_stats(bad)[keep], _stats(good)[keep])
    assert np.array_equal(_region_sums(bad)[keep], _region_sums(good)[keep])


# -- 6. end to end -------------------------------------------------------------------------------------------------------------------------
def _end_to_end(h, g, msh):
    u = h.solve()
    r = h.reconstruct(regions=True)
    e = g.reconstruct(u)  # the same coefficient as a plain callable: element means sampled on the host
    assert not r.info.any() and not e.info.any()
    for name in ("mean_flux", "energy", "max_flux"):
        a, b = getattr(r, name), getattr(e, name)
        print(name, np.abs(a - b).max() / np.abs(b).max())
        assert np.abs(a - b).max() < 1e-10 * np.abs(b).max(), name
    macro = u.x.array @ (h._A @ u.x.array)
    assert abs(msh.cell_volumes() @ r.energy - macro) < 1e-10 * abs(macro)
    assert r.region_volume.shape == (msh.num_cells, 2) and np.all(r.region_volume > 0)
    back = np.einsum("cr,crt->ct", r.region_volume, r.region_mean_flux)
    print("sum of regions", np.abs(back - r.mean_flux).max() / np.abs(r.mean_flux).max())
    assert np.abs(back - r.mean_flux).max() < 1e-12 * np.abs(r.mean_flux).max()
    assert np.array_equal(r.region_max_flux.max(axis=1), r.max_flux)
    return r


def test_poisson_hmm_end_to_end():
    msh, micro = Mm.create_unit_square(4, 4), Mm.create_unit_square(8, 8)
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.01 * (1.0 + 9.0 * x[0]), lambda x: 0.1 + 0.0 * x[0])
    h = hmm.PoissonHMM(msh, tp, lambda x: 1.0 + x[0], micro, 0.01)
    g = hmm.PoissonHMM(msh, lambda x, y: tp(x, y), lambda x: 1.0 + x[0], micro, 0.01, quadrature_degree=0)
    r = _end_to_end(h, g, msh)
    inside = np.asarray(tp.indicator(micro.cell_midpoints()[:, :2].T), dtype=bool)
    assert np.allclose(r.region_volume[:, 1], inside.mean(), rtol=1e-12)
    two = h.reconstruct(cells=[3, 20], regions=True, fields=True)
    assert np.array_equal(two.region_mean_flux, r.region_mean_flux[[3, 20]]) and np.array_equal(two.energy, r.energy[[3, 20]])
    assert np.allclose(two.region_mean_flux[:, 1], two.flux[:, inside].mean(axis=1), rtol=1e-11, atol=1e-14)


def test_elasticity_hmm_end_to_end():
    msh, micro = Mm.create_unit_cube(2, 2, 2), Mm.create_unit_cube(5, 5, 5)
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[1], y[2], 0.3), lambda x: hmm.Lame(2.0 + x[0], 10.0 + 5.0 * x[1]),
                      lambda x: hmm.Lame(1.0 + 0.0 * x[0], 0.5 + 0.0 * x[0]))
    load = lambda x: np.array([0.0, 0.0, -0.01])
    h = hmm.LinearElasticityHMM(msh, tp, load, micro, 0.05)
    g = hmm.LinearElasticityHMM(msh, lambda x, y: tp(x, y), load, micro, 0.05, quadrature_degree=0)
    V = h.function_space
    clamp = fem.locate_dofs_topological(V, 2, fem.locate_entities_boundary(msh, 2, lambda x: np.isclose(x[0], 0)))
    h.set_boundary_conditions(fem.dirichletbc(np.zeros(3), clamp, V))
    _end_to_end(h, g, msh)


if __name__ == "__main__":
    np.savez(sys.argv[1], **_chunk_case()[0])
