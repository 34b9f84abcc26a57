"""The derived-output kernels compute the bits they computed before they shared one geometry block, one reduction and one launcher
(-m gpu; DESIGN 3, "Element-walk kernels").

k_recon, k_sens, k_sens2_loads, k_sens2, k_sens_strat, k_polar and k_load_stats keep their arithmetic and the order of every addition: the
element loop, the "M, or the identity" preamble, the fixed-order sums and the max / argmax rule moved into elem_walk.h, nothing else.  So
every output must be the parent's, bit for bit.  tests/golden/elem_walk/parent_bits.npz was recorded on an MI355X with the parent build by
`python tests/test_gpu_elem_walk_bits.py OUT.npz`, from the same `compute()` the test runs; two recordings of the parent were array_equal.

Shapes, three seeded cells each, with and without M -- the smallest that reach every instantiation class: 2D Poisson n = 8 (fused route),
2D elasticity n = 5, 3D poisson_matrix n = 3, 3D elasticity n = 3 (the t = 6 rolled paths), and the jittered 2D Poisson and 3D
elasticity_voigt meshes of test_gpu_reconstruct.py::test_mesh_routes_match_reference as frontal plans with a load solve (the mesh path).
Outputs: reconstruct without fields, with fields and with three regions (one empty); sensitivities with shared directions, per-cell
directions and weights; second_sensitivities(first=True); stratification_sensitivities full and with weights; loads with response, fields
and correctors.  The per-element outputs (fields, the gradient of the weights, load correctors) are recorded at the 2D shapes alone, to
keep the fixture small; every array is held whole, so a failure shows which cell and entry moved.  One more case has a NaN cell.
"""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "elem_walk", "parent_bits.npz")  # a directory of its own: test_gpu_blocked counts golden/*.npz
NC = 3
SHAPES = {  # name -> (dim, kind, n or None for the mesh of that dimension)
    "p2": (2, "poisson", 8),
    "e2": (2, "elasticity", 5),
    "pm3": (3, "poisson_matrix", 3),
    "e3": (3, "elasticity", 3),
    "mesh_p2": (2, "poisson", None),
    "mesh_ev3": (3, "elasticity_voigt", None),
}
CASES = [(s, m) for s in SHAPES for m in (0, 1)]
NAN_SHAPE = "e2"


def _plan(shape):
    from hommx_amd import MicroCellPlan, workloads as W

    dim, kind, n = SHAPES[shape]
    if n:
        return MicroCellPlan(dim, n, kind)
    msh = W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)
    return MicroCellPlan.from_mesh(msh, kind, route="front", load_solve=True)


def _inputs(p, shape, with_M):
    import recon_ref as R

    dim, kind, _ = SHAPES[shape]
    rng = np.random.default_rng(7300 + 10 * list(SHAPES).index(shape) + with_M)
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    d = dict(
        coef=np.stack([R.random_coef(kind, dim, p.n_el, rng) for _ in range(NC)]),
        M=np.stack([R.random_M(dim, rng) for _ in range(NC)]) if with_M else None,
        xi=rng.standard_normal((NC, p.t)),
        dirs=rng.standard_normal((2,) + el),
        dirs_cell=rng.standard_normal((NC, 2) + el),
        weights=rng.standard_normal((NC, p.t, p.t)),
        labels=rng.integers(0, 3, p.n_el),  # 0, 1: regions; 2 -> 5: in no region, so that region 2 of three is empty
        P=rng.standard_normal(((NC,) if with_M else ()) + (2, p.n_el, p.t)),  # per cell with M, shared without
    )
    d["labels"][d["labels"] == 2] = 5
    return d


def _case(p, d, out, key, fields):
    """Every derived output of one plan and batch into out[key + name]; fields: the per-element outputs as well."""

    def put(name, a):
        out[key + name] = np.ascontiguousarray(a)

    def stats(r):
        return np.concatenate([r.mean_strain, r.mean_flux, r.energy[:, None], r.max_flux[:, None], r.argmax_element[:, None]], axis=1)

    coef, M = d["coef"], d["M"]
    r = p.reconstruct(coef, d["xi"], M)
    put("A", r.A_eff)
    put("info", r.info)
    put("recon_stats", stats(r))
    if fields:
        r = p.reconstruct(coef, d["xi"], M, fields=True)
        put("recon_fields_stats", stats(r))
        put("recon_strain", r.strain)
        put("recon_flux", r.flux)
    r = p.reconstruct(coef, d["xi"], M, regions=d["labels"], n_regions=3)
    put("recon_regions_stats", stats(r))
    some = r.region_volume[..., None] > 0  # the means of the empty region are NaN by definition: held as 0
    put("recon_regions", np.concatenate([r.region_volume[..., None], np.where(some, r.region_mean_strain, 0.0),
                                         np.where(some, r.region_mean_flux, 0.0), r.region_energy[..., None], r.region_max_flux[..., None],
                                         r.region_argmax_element[..., None]], axis=2))
    put("sens_dA", p.sensitivities(coef, M, directions=d["dirs"]).dA)
    put("sens_dA_cell", p.sensitivities(coef, M, directions=d["dirs_cell"], per_cell=True).dA)
    if fields:
        put("sens_grad", p.sensitivities(coef, M, weights=d["weights"]).grad)
    r = p.second_sensitivities(coef, M, directions=d["dirs"], first=True)
    put("sens2_d2A", r.d2A)
    put("sens2_dA", r.dA)
    put("strat_dA_dM", p.stratification_sensitivities(coef, M, full=True).dA_dM)
    put("strat_grad_M", p.stratification_sensitivities(coef, M, weights=d["weights"], full=False).grad_M)
    r = p.loads(coef, d["P"], M, response=True, fields=fields, return_correctors=fields)
    put("loads_P_eff", r.P_eff)
    put("loads_energy", r.energy)
    put("loads_stats", np.concatenate([r.mean_flux, r.max_flux[..., None], r.argmax_element[..., None]], axis=2))
    if fields:
        put("loads_strain", r.strain)
        put("loads_flux", r.flux)
        put("loads_correctors", r.correctors)


def compute():
    """name -> array: everything the fixture holds, computed by the build under test."""
    out = {}
    for shape in SHAPES:
        p = _plan(shape)
        for with_M in (0, 1):
            _case(p, _inputs(p, shape, with_M), out, f"{shape}_M{with_M}_", fields=p.dim == 2)
        if shape == NAN_SHAPE:
            d = _inputs(p, shape, 1)
            d["coef"][1, 7, 0] = np.nan
            _case(p, d, out, f"{shape}_nan_", fields=False)
        p.close()
    return out


@pytest.fixture(scope="module")
def got():
    return compute()


@pytest.fixture(scope="module")
def want():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(got, want):
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("shape,with_M", CASES)
def test_derived_output_bits(shape, with_M, got, want):
    key = f"{shape}_M{with_M}_"
    names = [k for k in want if k.startswith(key)]
    assert len(names) == (21 if SHAPES[shape][0] == 2 else 14)
    assert not want[key + "info"].any()
    for k in names:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_nan_cell_bits(got, want):
    key = f"{NAN_SHAPE}_nan_"
    names = [k for k in want if k.startswith(key)]
    assert len(names) == 14
    info = want[key + "info"]
    assert info[1] > 0 and not info[[0, 2]].any()
    assert np.isnan(want[key + "recon_stats"][1]).any()
    for k in names:
        assert np.array_equal(got[k][[0, 2]], want[k][[0, 2]]), k
        assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), k


if __name__ == "__main__":  # record the fixture with the build that is loaded (the parent's)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    np.savez_compressed(sys.argv[1], **compute())
    print("recorded", sys.argv[1], os.path.getsize(sys.argv[1]), "bytes")
