"""Strain-dependent coefficients: the secant iteration on the device (-m gpu; csrc/secant.hip, hommx_secant_source).

The shapes are those of test_gpu_elem_walk_bits.py, three seeded cells each, with and without M: every (DIM, KIND, MESH) class of
k_secant_update.  Three things are held:

* the evaluation of the law and the commit, bit for bit: ``SecantLaw.host_values`` fed with the strain, the flux and the base
  coefficient of the same call reproduces ``values`` for a program of exactly rounded operations; the committed stream is
  ``add_rn(mul_rn(1 - relax, c), mul_rn(relax, v))``;
* the iteration against tests/secant_ref.py (the same rounds on the correctors of an independent solver): 1e-9 relative after four
  rounds, the bound of the project between device and float64 references of derived outputs; the rounds to ``tol = 1e-10`` within one;
  closed forms;
* what the header promises of a stopped cell: its outputs belong together and do not depend on the chunking, the batch position,
  ``max_iter`` beyond its own stopping round, the outputs asked for or the entry.

The laws.  ``SOFT = 0.5 + 0.5 / (1 + e0^2 + e1^2)`` scales every entry of the base coefficient on the kinds with up to six entries (so
the tensor stays positive definite: a positive multiple of the base); on the Voigt kind the 128 instructions of a program do not hold 21
such entries, so the six diagonal entries are scaled by ``1 + 0.5 / (1 + e0^2)`` (the base plus a positive diagonal matrix) and the
others copied.  For the scalar law s -> s a(s) is increasing (its derivative is at least 0.4375); the references of all six shapes stop
with status 0 well inside 60 rounds (checked on the CPU with secant_ref; the rounds are printed by the convergence test).
"""

import functools

import numpy as np
import pytest

from test_gpu_criterion import EXACT
from test_gpu_elem_walk_bits import NC, SHAPES, _inputs

pytestmark = pytest.mark.gpu

CASES = [(s, m) for s in SHAPES for m in (0, 1)]
SOFT = "(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"
VOIGT_DIAGONAL = (0, 6, 11, 15, 18, 20)  # of the 21 entries, the upper triangle of the 6 x 6 tensor row by row
N_COMP = {"poisson": lambda d: 1, "poisson_matrix": lambda d: d * (d + 1) // 2, "elasticity": lambda d: 2, "elasticity_voigt": lambda d: 21 if d == 3 else 6}


def _law(texts, **kw):
    """A SecantLaw from the flat list of its component texts, in the shape the kind takes."""
    from hommx_amd.expr import SecantLaw

    n, matrix = len(texts), kw.pop("matrix", False)
    if n == 1:
        return SecantLaw(texts[0], **kw)
    if n == 2:
        return SecantLaw(lam=texts[0], mu=texts[1], **kw)
    if n == 3:
        return SecantLaw([[texts[0], texts[2]], [texts[2], texts[1]]], **kw)
    if n == 6 and matrix:
        a = texts
        return SecantLaw([[a[0], a[3], a[4]], [a[3], a[1], a[5]], [a[4], a[5], a[2]]], **kw)
    return SecantLaw(list(texts), **kw)


def soft_law(kind, dim, scale="", **kw):
    """The softening law of the module docstring for a kind; ``scale``: a text every component is multiplied with in front."""
    n = N_COMP[kind](dim)
    if n == 21:
        return _law([f"{scale}c[{k}]*(1 + 0.5/(1 + e[0]**2))" if k in VOIGT_DIAGONAL else f"{scale}c[{k}]" for k in range(n)], **kw)
    return _law([f"{scale}c[{k}]*{SOFT}" for k in range(n)], matrix=kind == "poisson_matrix", **kw)


def exact_law(kind, dim):
    """Exactly rounded operations only, reading x y p f e s c: component 0 is EXACT of test_gpu_criterion.py, component k adds one
    product of the state to its own base entry; of the 21 Voigt entries those from 6 on are a product (even k) or a copy (odd k) --
    the 128 instructions hold EXACT (47 of them) once."""
    n = N_COMP[kind](dim)
    rest = [f"c[{k}]*s[{k % 2}] - e[{(k + 1) % 2}]" if k < 6 else f"c[{k}]*s[0]" if k % 2 == 0 else f"c[{k}]" for k in range(1, n)]
    return _law([EXACT] + rest, p=[0.75], fields=1, matrix=kind == "poisson_matrix")


@functools.lru_cache(maxsize=None)
def _plan(shape):
    from hommx_amd import MicroCellPlan, workloads as W

    dim, kind, n = SHAPES[shape]
    if n:
        return MicroCellPlan(dim, n, kind)
    msh = W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)
    return MicroCellPlan.from_mesh(msh, kind, route="front", load_solve=True)


def _solver(shape):
    import secant_ref as S
    from hommx_amd import workloads as W

    dim, kind, n = SHAPES[shape]
    if n:
        return S.solver(kind, dim, n)
    return S.solver(kind, dim, msh=W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3))


@functools.lru_cache(maxsize=None)
def _case(shape, with_M):
    """The inputs of test_gpu_elem_walk_bits.py and, seeded, what a law reads beside them: rows (midpoint, one field) and points."""
    p = _plan(shape)
    d = _inputs(p, shape, with_M)
    rng = np.random.default_rng(9400 + 10 * list(SHAPES).index(shape) + with_M)
    d["rows"] = rng.integers(-8, 9, (NC, 4)) / 8.0  # dyadic: the comparisons on x and f are decided alike on both sides
    d["points"] = rng.integers(0, 17, (p.n_el, p.dim)) / 16.0
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p, d


def _run(p, d, law, **kw):
    rows = d["rows"][:, :3 + law.n_fields]
    return p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, points=d["points"], **kw)


def _bits(r):
    """What the header promises bit for bit of a stopped cell."""
    return [r.rounds, r.change, r.status, r.A_eff, r.mean_flux, r.coef, r.info]


def _same(a, b, cells=slice(None), what=""):
    for x, y in zip(_bits(a), _bits(b)):
        if x is not None and y is not None:
            assert np.array_equal(x[cells], y[cells], equal_nan=x.dtype.kind == "f"), what


def _check_consistent(p, d, r, what):
    """Item 3: the outputs of the stopping round belong together.  ``solve`` may run another route than the correctors' (1e-12);
    ``reconstruct`` eliminates on the same one (bitwise)."""
    A = p.solve(r.coef, d["M"])
    ok = r.status != 3  # a flagged pivot: A_eff may hold anything
    dev = np.abs(A - r.A_eff)[ok].max() / np.abs(r.A_eff[ok]).max()
    gap = np.abs(r.mean_flux - np.einsum("cij,cj->ci", r.A_eff, d["xi"]))[ok]
    bound = (1e-12 * np.linalg.norm(r.A_eff.reshape(NC, -1), axis=1) * np.linalg.norm(d["xi"], axis=1))[ok]
    print(f"{what}: |solve(coef) - A_eff| = {dev:.3e} of the largest entry; |mean_flux - A_eff xi| = {gap.max():.3e}, bound {bound.min():.3e}")
    assert dev <= 1e-12, what
    assert np.all(gap.max(axis=1) <= bound), what
    same_route = p.reconstruct(r.coef, d["xi"], d["M"])  # the corrector route of the plan, the one the iteration eliminates on: bitwise
    assert np.array_equal(same_route.A_eff[ok], r.A_eff[ok]) and np.array_equal(same_route.info, r.info), what


# -- 1. the program, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_exact_program_equals_the_host_twin_bitwise(shape, with_M):
    p, d = _case(shape, with_M)
    law = exact_law(p.kind, p.dim)
    r = _run(p, d, law, max_iter=1, fields=True, values=True, return_coef=True)
    assert not r.info.any() and np.array_equal(r.rounds, np.ones(NC, dtype=np.int64))
    host = law.host_values(r.strain, r.flux, d["coef"], d["rows"][:, :3], d["points"], d["rows"][:, 3:4])
    assert r.values.shape == host.shape == (NC, p.n_el, p.n_comp)
    assert np.array_equal(r.values, host)
    assert np.array_equal(r.coef, d["coef"])  # a stopping round commits nothing
    ref = p.reconstruct(d["coef"], d["xi"], d["M"], fields=True)
    for name in ("strain", "flux"):
        got, want = getattr(r, name), getattr(ref, name)
        dev = np.abs(got - want).max() / np.abs(want).max()
        print(f"{shape} M{with_M} {name}: deviation from reconstruct {dev:.3e} of the largest entry")
        assert dev <= 1e-9
    assert np.array_equal(r.A_eff, ref.A_eff)


# -- 2. the commit, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_commit_arithmetic_bitwise(shape, with_M):
    p, d = _case(shape, with_M)
    law = soft_law(p.kind, p.dim)
    v = _run(p, d, law, max_iter=1, values=True).values.reshape(d["coef"].shape)
    half = _run(p, d, law, max_iter=2, tol=0.0, relax=0.5, return_coef=True)
    assert np.array_equal(half.coef, 0.5 * d["coef"] + 0.5 * v)  # NumPy: the products and the sum separately rounded
    full = _run(p, d, law, max_iter=2, tol=0.0, relax=1.0, return_coef=True)
    assert np.array_equal(full.coef, v)
    assert np.array_equal(full.rounds, np.full(NC, 2)) and np.array_equal(full.status, np.ones(NC, dtype=np.int64))
    again = _run(p, d, law, max_iter=1, coef_start=full.coef, return_coef=True)
    assert np.array_equal(again.A_eff, full.A_eff) and np.array_equal(again.coef, full.coef)
    _check_consistent(p, d, half, f"{shape} M{with_M} relax 0.5")
    _check_consistent(p, d, full, f"{shape} M{with_M} relax 1")


# -- 4. / 5. the iteration against the reference -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(shape, max_iter, tol):
    """secant_ref on the three cells of `shape` with M: computed once, read only."""
    import secant_ref as S

    p, d = _case(shape, 1)
    law, solve = soft_law(p.kind, p.dim), _solver(shape)
    return [S.iterate(solve, law, d["coef"][c], d["xi"][c], d["M"][c], max_iter=max_iter, tol=tol) for c in range(NC)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_four_rounds_against_the_reference(shape):
    p, d = _case(shape, 1)
    r = _run(p, d, soft_law(p.kind, p.dim), max_iter=4, tol=0.0, return_coef=True)
    ref = _reference(shape, 4, 0.0)
    assert np.array_equal(r.rounds, np.full(NC, 4)) and np.array_equal(r.status, np.ones(NC, dtype=np.int64)) and not r.info.any()
    for c in range(NC):
        dc = np.abs(r.coef[c] - ref[c]["coef"]).max() / np.abs(ref[c]["coef"]).max()
        dA = np.abs(r.A_eff[c] - ref[c]["A"]).max() / np.abs(ref[c]["A"]).max()
        print(f"{shape} cell {c}: fourth iterate, coef {dc:.3e}, A_eff {dA:.3e} (relative to the largest entry)")
        assert dc <= 1e-9 and dA <= 1e-9
    _check_consistent(p, d, r, f"{shape} four rounds")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_convergence_in_the_rounds_of_the_reference(shape):
    p, d = _case(shape, 1)
    r = _run(p, d, soft_law(p.kind, p.dim), max_iter=60, tol=1e-10, return_coef=True)
    ref = _reference(shape, 60, 1e-10)
    print(f"{shape}: rounds {r.rounds.tolist()} against {[x['rounds'] for x in ref]} of the reference; change {r.change.tolist()}")
    assert all(x["status"] == 0 for x in ref)  # the law and the strains were chosen for this
    assert not r.status.any() and not r.info.any()
    assert np.all(np.abs(r.rounds - np.array([x["rounds"] for x in ref])) <= 1)
    assert np.all(r.change <= 1e-10)
    _check_consistent(p, d, r, f"{shape} converged")


# -- 6. closed forms ----------------------------------------------------------------------------------------------------------------------
def test_homogeneous_poisson_is_the_law_at_the_macro_gradient():
    p = _plan("p2")
    xi = np.array([[1.5, 0.5], [0.1, 0.0], [5.0, -3.0]])
    r = p.secant(np.ones((NC, p.n_el)), xi, _law([SOFT[1:-1]]), max_iter=10, tol=1e-14)
    a = 0.5 + 0.5 / (1 + (xi**2).sum(axis=1))
    assert np.array_equal(r.rounds, np.full(NC, 2)) and not r.status.any() and np.all(r.change <= 1e-14)
    assert np.abs(r.A_eff - a[:, None, None] * np.eye(2)).max() <= 1e-12


def test_homogeneous_elasticity_is_the_tensor_of_the_softened_shear_modulus():
    import periodic_fem as PF

    p = _plan("e3")
    rng = np.random.default_rng(5)
    xi = rng.standard_normal((NC, 6))
    lam, mu0 = 2.0, 1.5
    base = np.broadcast_to(np.array([lam, mu0]), (NC, p.n_el, 2)).copy()
    r = p.secant(base, xi, _law(["c[0]", f"c[1]*{SOFT}"]), max_iter=10, tol=1e-14)
    assert np.array_equal(r.rounds, np.full(NC, 2)) and not r.status.any() and np.all(r.change <= 1e-14)
    mu = mu0 * (0.5 + 0.5 / (1 + xi[:, 0] ** 2 + xi[:, 1] ** 2))
    for c in range(NC):
        C4 = PF.material_tensor("elasticity", np.array([[lam, mu[c]]]), 3)[0]
        C = np.array([[C4[i, j, k, l] for (k, l) in PF.PAIRS[3]] for (i, j) in PF.PAIRS[3]])
        assert np.abs(r.A_eff[c] - C).max() <= 1e-12 * np.abs(C).max()


def test_laminate_against_the_scalar_layer_equations():
    """b = 10 on y0 < 0.25, else 1, xi = (2, 0): the gradient is constant per layer, theta e1 + (1 - theta) e2 = 2 and
    b1 a(e1) e1 = b2 a(e2) e2 (the normal flux is continuous); A_H[0][0] = b1 a(e1) e1 / 2.  The issue records 0.7375971568671663."""
    from scipy.optimize import brentq

    from oracle import hommx_oracle as O

    p = _plan("p2")
    x, cells = O.unit_cell_mesh(2, 8)
    base = np.where(x[cells].mean(axis=1)[:, 0] < 0.25, 10.0, 1.0)
    a = lambda s: 0.5 + 0.5 / (1 + s * s)
    theta = 0.25
    e2_of = lambda e1: (2.0 - theta * e1) / (1 - theta)
    e1 = brentq(lambda e: 10.0 * a(e) * e - a(e2_of(e)) * e2_of(e), 0.0, 2.0, xtol=1e-15, rtol=1e-15)
    want = 10.0 * a(e1) * e1 / 2.0
    assert abs(want - 0.7375971568671663) <= 1e-11  # the recorded figure, to the tolerance of its root finder
    r = p.secant(base[None], np.array([[2.0, 0.0]]), soft_law("poisson", 2), max_iter=60, tol=1e-12)
    print(f"laminate: A_H[0][0] = {r.A_eff[0, 0, 0]!r} after {r.rounds[0]} rounds; layer equations {want!r}")
    assert r.status[0] == 0
    assert abs(r.A_eff[0, 0, 0] - want) <= 1e-9
    across = p.secant(base[None], np.array([[0.0, 2.0]]), soft_law("poisson", 2), max_iter=60, tol=1e-12)
    assert across.rounds[0] == 2 and across.status[0] == 0  # along the layers the gradient is xi everywhere


# -- 7. independence, bit for bit -------------------------------------------------------------------------------------------------------
def _staggered(shape):
    """The batch of `shape` with M, its macro strains scaled by 0.1, 1 and 3: the cells stop in different rounds."""
    p, d = _case(shape, 1)
    return p, dict(d, xi=d["xi"] * np.array([0.1, 1.0, 3.0])[:, None])


@pytest.mark.parametrize("shape", ["p2", "e3", "mesh_p2"])
def test_a_cell_does_not_depend_on_chunking_position_max_iter_or_outputs(shape, monkeypatch):
    p, d = _staggered(shape)
    law = soft_law(p.kind, p.dim)
    want = _run(p, d, law, max_iter=60, return_coef=True)
    print(f"{shape}: rounds {want.rounds.tolist()}")
    assert not want.status.any() and len(set(want.rounds.tolist())) > 1
    _check_consistent(p, d, want, f"{shape} staggered")
    _same(_run(p, d, law, max_iter=60, return_coef=True, fields=True, values=True), want, what="outputs")
    _same(_run(p, d, law, max_iter=60), want, what="no optional output")
    early = want.rounds < 25
    assert early.any()
    _same(_run(p, d, law, max_iter=25, return_coef=True), want, early, "max_iter")
    one = p.secant(d["coef"][1:2], d["xi"][1:2], law, d["M"][1:2], rows=d["rows"][1:2, :3], max_iter=60, return_coef=True)
    for x, y in zip(_bits(one), _bits(want)):
        assert np.array_equal(x[0], y[1])
    order = [2, 0, 1]
    swapped = p.secant(d["coef"][order], d["xi"][order], law, d["M"][order], rows=d["rows"][order, :3], max_iter=60, return_coef=True)
    for x, y in zip(_bits(swapped), _bits(want)):
        assert np.array_equal(x, y[order])
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")
    _plan.cache_clear()  # the variable is read when a plan is created
    try:
        q = _plan(shape)
        rep = 120  # 360 cells: at least two chunks of 1 MB of correctors (3.9 KiB per cell at the smallest shape)
        got = q.secant(np.concatenate([d["coef"]] * rep), np.concatenate([d["xi"]] * rep), law, np.concatenate([d["M"]] * rep), max_iter=60,
                       return_coef=True)
        for x, y in zip(_bits(got), _bits(want)):
            assert np.array_equal(x, np.concatenate([y] * rep))
        q.close()
    finally:
        _plan.cache_clear()
        _case.cache_clear()


@pytest.mark.parametrize("shape", ["p2", "e2", "mesh_ev3"])
def test_device_entry_equals_host_entry(shape):
    import torch

    from hommx_amd.batch import CoefStream

    p, d = _staggered(shape)
    law = soft_law(p.kind, p.dim)
    want = _run(p, d, law, max_iter=60, return_coef=True, fields=True, values=True)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    out = {"state": empty(NC, 3), "A_eff": empty(NC, p.t, p.t), "mean_flux": empty(NC, p.t), "coef": empty(*d["coef"].shape),
           "strain": empty(NC, p.n_el, p.t), "flux": empty(NC, p.n_el, p.t), "values": empty(NC, p.n_el, p.n_comp),
           "info": empty(NC, dtype=torch.int32)}
    ptr = {k: v.data_ptr() for k, v in out.items()}
    p.secant_device(NC, CoefStream.sampled(d["coef"]).coef_source(upload), upload(d["M"]), upload(d["xi"]), law, upload(d["rows"][:, :3]),
                    ptr["state"], ptr["A_eff"], max_iter=60, mean_flux_ptr=ptr["mean_flux"], coef_ptr=ptr["coef"], strain_ptr=ptr["strain"],
                    flux_ptr=ptr["flux"], values_ptr=ptr["values"], info_ptr=ptr["info"], stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["state"], np.stack([want.rounds, want.change, want.status], axis=1).astype(np.float64))
    for k in ("A_eff", "mean_flux", "coef", "strain", "flux", "values", "info"):
        assert np.array_equal(got[k], getattr(want, k)), k


# -- 8. the other statuses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_status_one_after_max_iter(shape, with_M):
    p, d = _case(shape, with_M)
    r = _run(p, d, soft_law(p.kind, p.dim), max_iter=3, tol=1e-15, return_coef=True)
    assert np.array_equal(r.status, np.ones(NC, dtype=np.int64)) and np.array_equal(r.rounds, np.full(NC, 3)) and np.all(r.change > 1e-15)
    _check_consistent(p, d, r, f"{shape} M{with_M} status 1")


@pytest.mark.parametrize("shape", ["p2", "e2"])
def test_a_value_that_is_not_finite_stops_its_cell_alone(shape):
    p, d = _staggered(shape)
    texts = soft_law(p.kind, p.dim).texts
    law = _law([f"{t} + 1e-300/(f[0] - 1)" for t in texts], fields=1)
    rows = np.concatenate([d["rows"][:, :3], np.zeros((NC, 1))], axis=1)
    want = p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, max_iter=60, return_coef=True)
    assert not want.status.any()
    rows[1, 3] = 1.0
    r = p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, max_iter=60, return_coef=True)
    assert r.status.tolist() == [0, 2, 0] and r.rounds[1] == 1
    assert np.array_equal(r.coef[1], d["coef"][1])  # the iterate before: the start
    _same(r, want, [0, 2], "the other cells")
    _check_consistent(p, d, r, f"{shape} status 2")


@pytest.mark.parametrize("shape", ["p2", "e2"])
def test_a_negative_coefficient_is_a_flagged_pivot(shape):
    p, d = _staggered(shape)
    law = soft_law(p.kind, p.dim, scale="f[0]*", fields=1)
    rows = np.concatenate([d["rows"][:, :3], np.ones((NC, 1))], axis=1)
    want = p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, max_iter=60, return_coef=True)
    assert not want.status.any()
    rows[1, 3] = -1.0
    r = p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, max_iter=60, return_coef=True)
    assert r.status.tolist() == [0, 3, 0] and r.info[1] != 0 and not r.info[[0, 2]].any()
    assert r.rounds[1] == 2 and np.all(r.coef[1] < 0)  # the stream the failed elimination read: every entry times -1
    _same(r, want, [0, 2], "the other cells")


# -- 9. the slot path: a field that does not fit LDS beside the stack ----------------------------------------------------------------------
def test_slot_path_and_lds_path_on_a_large_cell():
    from hommx_amd import MicroCellPlan

    n = 112  # 8 ndof = 98 KiB: with the 60 KiB of fifteen stack rows above the 150 KiB limit of the reconstruction, with one row below it
    p = MicroCellPlan(2, n, "poisson")
    rng = np.random.default_rng(12)
    d = {"coef": np.exp(rng.uniform(-1, 1, (1, p.n_el))), "xi": rng.standard_normal((1, 2)), "M": None,
         "rows": rng.integers(-8, 9, (1, 4)) / 8.0, "points": rng.integers(0, 17, (p.n_el, 2)) / 16.0}
    text = "e[0]**2"
    for _ in range(13):
        text = f"(1 + {text})"
    deep, shallow = _law([f"c[0]/{text}"]), _law(["c[0]/(1 + e[0]**2)"])
    assert deep.depth == 16 and shallow.depth <= 4 and 8 * n * n + 4096 * 15 > 150 * 1024 >= 8 * n * n + 4096 * 3
    for name, law in (("slot", deep), ("lds", shallow)):
        r = _run(p, d, law, max_iter=2, tol=0.0, fields=True, values=True, return_coef=True)
        assert not r.info.any() and r.rounds[0] == 2 and r.status[0] == 1
        first = _run(p, d, law, max_iter=1, fields=True, values=True)
        assert np.array_equal(first.values, law.host_values(first.strain, first.flux, d["coef"], d["rows"][:, :3])), name
        assert np.array_equal(r.coef, first.values[..., 0]), name
        assert np.array_equal(r.values, law.host_values(r.strain, r.flux, d["coef"], d["rows"][:, :3])), name
        A = p.solve(r.coef)
        assert np.abs(A - r.A_eff).max() <= 1e-12 * np.abs(A).max(), name
        assert np.abs(r.mean_flux[0] - r.A_eff[0] @ d["xi"][0]).max() <= 1e-12 * np.linalg.norm(r.A_eff[0]) * np.linalg.norm(d["xi"][0]), name
    p.close()


# -- 11. the solver classes ---------------------------------------------------------------------------------------------------------------
def test_solve_nonlinear_with_the_identity_law_is_solve():
    from hommx_amd import hmm, mesh

    A = hmm.TwoPhase(lambda y: (y[0] - 0.5) ** 2 + (y[1] - 0.5) ** 2 < 0.09, lambda x: 10.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(6, 6), A, lambda x: 1.0 + 0.0 * x[0], mesh.create_unit_square(8, 8), 0.05)
    u = h.solve().x.array.copy()
    v = h.solve_nonlinear(hmm.SecantLaw("c[0]")).x.array
    assert len(h.nonlinear_history) == 1 and h.nonlinear_history[0] <= 1e-12
    assert np.abs(u - v).max() <= 1e-12 * np.abs(u).max()
    assert np.array_equal(h.secant.rounds, np.ones(len(h.secant.rounds), dtype=np.int64)) and not h.secant.status.any()  # v = c: no change


def test_poisson_hmm_follows_the_kacanov_loop_of_the_macro_problem():
    """A homogeneous micro coefficient: the secant tensor of a cell is a(|grad u|) I exactly, so every macro iterate must be that of
    the Kacanov loop of -div(a(|grad u|) grad u) = 1 on P1 elements, assembled here from per-cell scalars."""
    from hommx_amd import hmm, mesh

    h = hmm.PoissonHMM(mesh.create_unit_square(6, 6), lambda x, y: 1.0 + 0.0 * x[0] * y[0], lambda x: 40.0 + 0.0 * x[0],
                       mesh.create_unit_square(4, 4), 0.05)
    law = hmm.SecantLaw(f"c[0]*{SOFT}")
    u = h.solve().x.array.copy()
    cells = np.arange(h._msh.num_cells)
    for k in range(1, 6):
        xi = h._macro_strains(cells, u)
        a = 0.5 + 0.5 / (1 + (xi**2).sum(axis=1))
        h._set_macro_matrix(h._local_stiffness_from_tensors(cells, a[:, None, None] * np.eye(2)))
        u = h.solve().x.array.copy()
        h._needs_reassembly = True  # solve_nonlinear starts from the linear solve()
        got = h.solve_nonlinear(law, max_iter=k, tol=0.0).x.array
        dev = np.abs(got - u).max() / np.abs(u).max()
        print(f"macro iterate {k}: deviation from the Kacanov loop {dev:.3e}")
        assert dev <= 1e-10
    assert len(h.nonlinear_history) == 5 and h.nonlinear_history[0] > 1e-3  # the load is large enough for the law to matter


def test_stratified_elasticity_converges_to_a_solution_of_its_own_secant_system():
    from hommx_amd import fem, hmm, mesh

    A = hmm.TwoPhase(lambda y: y[0] < 0.5, lambda x: hmm.Lame(20.0 + 0.0 * x[0], 10.0 + 0.0 * x[0]),
                     lambda x: hmm.Lame(2.0 + 0.0 * x[0], 1.0 + 0.0 * x[0]))
    h = hmm.LinearElasticityStratifiedHMM(mesh.create_unit_square(4, 4), A, lambda x: np.array([0.0, -8.0]), mesh.create_unit_square(5, 5), 0.05,
                                          lambda x: np.array([[1.0, 0.1], [0.2, 0.9]]))
    V = h.function_space
    clamp = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1) | np.isclose(x[1], 0) | np.isclose(x[1], 1))
    h.set_boundary_conditions(fem.dirichletbc(fem.Function(V), clamp, V))
    tol = 1e-8
    u = h.solve_nonlinear(hmm.SecantLaw(lam="c[0]", mu=f"c[1]*{SOFT}"), max_iter=40, tol=tol).x.array.copy()
    assert h.nonlinear_history[-1] <= tol and len(h.nonlinear_history) > 2 and not h.secant.status.any()
    h._set_macro_matrix(h._local_stiffness_from_tensors(np.arange(h._msh.num_cells), h.effective_tensors))
    v = h.solve().x.array
    dev = np.abs(u - v).max() / np.abs(v).max()
    print(f"stratified elasticity: {len(h.nonlinear_history)} macro steps, |u - solve(secant tensors)| = {dev:.3e}")
    assert dev <= 10 * tol
