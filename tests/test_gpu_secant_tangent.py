"""The consistent tangent of the secant response on the device (-m gpu; csrc/secant_tangent.hip, hommx_secant_tangent_source;
DESIGN 4.16), on the shapes of test_gpu_elem_walk_bits.py, three seeded cells each, with and without M: every (DIM, KIND, MESH) class
of k_secant_tangent.  Held:

* every output shared with ``secant()`` has its bits;
* the tangent coefficient, bit for bit: ``SecantLaw.host_tangent`` fed with the strain and the stream of the same call reproduces
  ``tangent_coef`` for a law of exactly rounded operations that reads x y p f e c; the tangent is the sibling plan's ``solve`` of it;
* D against tests/secant_tangent_ref.py (the reference's iteration to tol = 1e-12, the analytic element tangent, the reference's solver
  of the tangent kind): 1e-9 of the largest entry, the bound of the project between device and float64 references;
* a cell does not depend on the chunking, the batch position, ``max_iter`` beyond its stopping round, the outputs asked for or the entry; a cell of
  status 2 or 3 has NaN tangent and asymmetry and leaves the others alone; the asymmetry of a law without a potential is the
  reference's; a deep program takes the P = 1 sweeps and agrees with the twin; Newton reaches the secant solution in fewer steps.

The potential laws are those of secant_tangent_ref.py; they stop with status 0 well inside 60 rounds (test_secant_tangent_host.py).
"""

import functools

import numpy as np
import pytest

import secant_tangent_ref as TR
from test_gpu_elem_walk_bits import NC, SHAPES
from test_gpu_secant import CASES, _bits, _case, _law, _plan, _run

pytestmark = pytest.mark.gpu


def _mesh(dim):
    from hommx_amd import workloads as W

    return W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)


@functools.lru_cache(maxsize=None)
def _sibling(shape):
    from hommx_amd import MicroCellPlan

    dim, kind, n = SHAPES[shape]
    p = _plan(shape)
    return MicroCellPlan(dim, n, p.tangent_kind) if n else MicroCellPlan.from_mesh(_mesh(dim), p.tangent_kind, route="front")


def _tangent(p, d, law, shape, **kw):
    rows = d["rows"][:, :3 + law.n_fields]
    return p.secant_tangent(d["coef"], d["xi"], law, _sibling(shape), d["M"], rows=rows, points=d["points"], **kw)


def _stream(shape, T):
    """T[N, n_el, t, t] of the twin as the element stream of the tangent kind, in the order secant_tangent_ref.py writes down."""
    dim, kind, _ = SHAPES[shape]
    return np.stack([TR.tangent_stream(kind, dim, T[c]) for c in range(len(T))])


def _tbits(r):
    return _bits(r) + [r.tangent, r.asymmetry, r.tangent_info, r.tangent_coef]


def _same(a, b, cells=slice(None), what=""):
    for x, y in zip(_tbits(a), _tbits(b)):
        if x is not None and y is not None:
            assert np.array_equal(x[cells], y[cells], equal_nan=x.dtype.kind == "f"), what


def exact_explicit_law(kind, dim):
    """Exactly rounded operations only (+ - * / abs min), reading x y p f e c and no s: the first component takes all of them, the
    others soften their own base entry with one strain entry; of the 21 Voigt entries the fifteen off the diagonal are copies."""
    t, n = TR.tensor_size(kind, dim), TR.N_COMP[kind](dim)
    first = "c[0]*(p[0] + 0.25/(1 + min(e[0]**2, 4.0) + f[0]**2*abs(e[1]) + abs(x[0])*y[0]*y[1]))"
    diagonal = {k for k, (r, c) in enumerate(TR.entries(kind, dim)) if r == c} if kind == "elasticity_voigt" else set(range(n))
    rest = [f"c[{k}]*(1 + 0.25/(1 + e[{k % t}]**2))" if k in diagonal else f"c[{k}]" for k in range(1, n)]
    return _law([first] + rest, p=[0.75], fields=1, matrix=kind == "poisson_matrix")


# -- 1. shared outputs, the twin, the sibling's solve -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_shared_outputs_are_those_of_secant_and_the_coefficient_is_the_twins(shape, with_M):
    p, d = _case(shape, with_M)
    law = exact_explicit_law(p.kind, p.dim)
    kw = dict(max_iter=3, tol=1e-3, fields=True, values=True, return_coef=True)
    want = _run(p, d, law, **kw)
    got = _tangent(p, d, law, shape, return_tangent_coef=True, **kw)
    for name in ("A_eff", "mean_flux", "rounds", "change", "status", "info", "coef", "strain", "flux", "values"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert set(np.unique(got.status)) <= {0, 1}
    T, asym = law.host_tangent(got.strain, got.coef, d["coef"], d["rows"][:, :3], d["points"], d["rows"][:, 3:4])
    assert np.array_equal(got.tangent_coef, _stream(shape, T)), "tangent_coef"
    assert np.array_equal(got.asymmetry, asym), "asymmetry"
    sib = _sibling(shape)
    D, info = sib.solve(got.tangent_coef, d["M"], return_info=True)
    ok = info == 0
    dev = np.abs(D - got.tangent)[ok].max() / np.abs(D[ok]).max()
    print(f"{shape} M={with_M}: route {sib.kernel}; tangent against solve(tangent_coef): {dev:.3e}, bitwise: {np.array_equal(D[ok], got.tangent[ok])}")
    assert np.array_equal(info, got.tangent_info) and ok.all()
    assert dev <= 1e-12
    assert np.array_equal(D, got.tangent)  # one internal function under both calls: the same launches on the same batch


# -- 2. against the float64 reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_tangent_against_the_reference(shape, with_M):
    dim, kind, n = SHAPES[shape]
    p, d = _case(shape, with_M)
    law, dlaw = TR.potential_law(kind, dim)
    got = _tangent(p, d, law, shape, max_iter=60, tol=1e-12)
    assert not got.status.any() and not got.tangent_info.any(), (got.status, got.tangent_info)
    worst = 0.0
    for c in range(NC):
        ref = TR.tangent(kind, dim, law, dlaw, d["coef"][c], d["xi"][c], None if d["M"] is None else d["M"][c], n=n,
                         msh=None if n else _mesh(dim), x=d["rows"][c, :3], y=d["points"], max_iter=60, tol=1e-12)
        assert ref["status"] == 0
        worst = max(worst, np.abs(got.tangent[c] - ref["D"]).max() / np.abs(ref["D"]).max())
        assert abs(got.rounds[c] - ref["rounds"]) <= 1
    print(f"{shape} M={with_M}: rounds {got.rounds}, |D - D_ref| = {worst:.3e} of the largest entry, asymmetry {got.asymmetry.max():.1e}")
    assert worst <= 1e-9
    assert np.all(got.asymmetry <= 1e-14)


# -- 3. what a cell does not depend on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_cell_does_not_depend_on_position_rounds_or_outputs(shape):
    dim, kind, _ = SHAPES[shape]
    p, d = _case(shape, 1)
    law, _ = TR.potential_law(kind, dim)
    full = _tangent(p, d, law, shape, max_iter=60, tol=1e-8, fields=True, values=True, return_coef=True, return_tangent_coef=True)
    assert not full.status.any()
    bare = _tangent(p, d, law, shape, max_iter=int(full.rounds.max()), tol=1e-8)  # no optional output, no round beyond the last stop
    _same(full, bare, what="outputs asked for / max_iter")
    perm = np.array([2, 0, 1])
    moved = dict(d, **{k: d[k][perm] for k in ("coef", "M", "xi", "rows")})
    again = _tangent(p, moved, law, shape, max_iter=60, tol=1e-8, return_coef=True, return_tangent_coef=True)
    for x, y in zip(_tbits(full), _tbits(again)):
        if x is not None and y is not None:
            assert np.array_equal(x[perm], y, equal_nan=x.dtype.kind == "f"), "batch position"


@pytest.mark.parametrize("shape", ["p2", "mesh_p2"])
def test_a_cell_does_not_depend_on_chunking(shape, monkeypatch):
    """360 cells through a plan of HOMMX_RECON_MEM_MB = 1 (read when the plan is created): at least two chunks of 1 MB of correctors
    (3.9 KiB per cell at the smallest shape), each with its own tangent launch and its own elimination on the sibling plan."""
    from hommx_amd import MicroCellPlan

    dim, kind, n = SHAPES[shape]
    p, d = _case(shape, 1)
    law, _ = TR.potential_law(kind, dim)
    want = _tangent(p, d, law, shape, max_iter=60, tol=1e-8, return_coef=True)
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")
    q = MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(_mesh(dim), kind, route="front", load_solve=True)
    try:
        rep = 120
        tile = lambda a: np.concatenate([a] * rep)
        got = q.secant_tangent(tile(d["coef"]), tile(d["xi"]), law, _sibling(shape), tile(d["M"]), rows=tile(d["rows"][:, :3]),
                               points=d["points"], max_iter=60, tol=1e-8, return_coef=True)
        for x, y in zip(_tbits(got), _tbits(want)):
            if x is not None and y is not None:
                assert np.array_equal(x, tile(y), equal_nan=x.dtype.kind == "f")
    finally:
        q.close()


@pytest.mark.parametrize("shape", ["p2", "e2", "mesh_ev3"])
def test_device_entry_equals_host_entry(shape):
    import torch

    from hommx_amd.batch import CoefStream

    dim, kind, _ = SHAPES[shape]
    p, d = _case(shape, 1)
    law, _ = TR.potential_law(kind, dim)
    want = _tangent(p, d, law, shape, max_iter=60, tol=1e-8, return_coef=True, return_tangent_coef=True)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    nt = p.t * (p.t + 1) // 2
    out = {"state": empty(NC, 3), "A_eff": empty(NC, p.t, p.t), "mean_flux": empty(NC, p.t), "coef": empty(*d["coef"].shape),
           "info": empty(NC, dtype=torch.int32), "tangent": empty(NC, p.t, p.t), "asymmetry": empty(NC), "tangent_coef": empty(NC, p.n_el, nt),
           "tangent_info": empty(NC, dtype=torch.int32)}
    ptr = {k: v.data_ptr() for k, v in out.items()}
    p.secant_tangent_device(NC, CoefStream.sampled(d["coef"]).coef_source(upload), upload(d["M"]), upload(d["xi"]), law, _sibling(shape),
                            upload(d["rows"][:, :3]), ptr["state"], ptr["A_eff"], ptr["tangent"], ptr["asymmetry"],
                            points_ptr=upload(d["points"]), max_iter=60, tol=1e-8, mean_flux_ptr=ptr["mean_flux"], coef_ptr=ptr["coef"],
                            info_ptr=ptr["info"], tangent_coef_ptr=ptr["tangent_coef"], tangent_info_ptr=ptr["tangent_info"],
                            stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["state"], np.stack([want.rounds, want.change, want.status], axis=1).astype(np.float64))
    for k in ("A_eff", "mean_flux", "coef", "info", "tangent", "asymmetry", "tangent_coef", "tangent_info"):
        assert np.array_equal(got[k], getattr(want, k)), k


# -- 4. the other statuses ------------------------------------------------------------------------------------------------------------------
def test_a_stopped_cell_of_status_2_or_3_is_nan_and_alone():
    """Cell 1: its field is 0 and the law divides by it (a value that is not finite, status 2); cell 2: a negative base coefficient
    (a flagged pivot, status 3).  Cell 0 keeps every bit of the run in which all three cells are sound."""
    from hommx_amd.expr import SecantLaw

    p, d = _case("p2", 1)
    law = SecantLaw("c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))/f[0]", fields=1)
    rows = np.concatenate([d["rows"][:, :3], np.ones((NC, 1))], axis=1)
    sound = dict(d, rows=rows)
    good = _tangent(p, sound, law, "p2", max_iter=60, tol=1e-8, return_coef=True, return_tangent_coef=True)
    assert not good.status.any()
    bad_rows, bad_coef = rows.copy(), d["coef"].copy()
    bad_rows[1, 3] = 0.0
    bad_coef[2] = -bad_coef[2]
    got = _tangent(p, dict(d, rows=bad_rows, coef=bad_coef), law, "p2", max_iter=60, tol=1e-8, return_coef=True, return_tangent_coef=True)
    assert list(got.status) == [0, 2, 3], got.status
    assert np.isnan(got.tangent[1:]).all() and np.isnan(got.asymmetry[1:]).all()
    identity = np.broadcast_to(np.array([1.0, 1.0, 0.0]), (p.n_el, 3))
    assert np.array_equal(got.tangent_coef[1], identity) and np.array_equal(got.tangent_coef[2], identity)
    _same(good, got, cells=slice(0, 1), what="the sound cell")


def test_the_asymmetry_of_a_law_without_a_potential_is_the_references():
    dim, kind, n = SHAPES["e2"]
    p, d = _case("e2", 0)
    law, dlaw = TR.potential_law(kind, dim, asymmetric=True)
    got = _tangent(p, d, law, "e2", max_iter=60, tol=1e-12)
    assert not got.status.any()
    for c in range(NC):
        ref = TR.tangent(kind, dim, law, dlaw, d["coef"][c], d["xi"][c], None, n=n, x=d["rows"][c, :3], y=d["points"], max_iter=60, tol=1e-12)
        print(f"cell {c}: asymmetry {got.asymmetry[c]:.6e}, reference {ref['asymmetry']:.6e}")
        assert ref["asymmetry"] > 1e-4 and abs(got.asymmetry[c] - ref["asymmetry"]) <= 1e-9


# -- 5. the P = 1 sweeps of a deep program --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["e2", "e3"])
def test_a_deep_program_takes_single_sweeps_and_agrees_with_the_twin(shape):
    """Depth 16: the stack rows of the wide sweep do not fit LDS, so every strain entry gets a sweep of its own.  The nesting is to the
    right, ``e0^2 + (a_1 + (a_2 + ...))`` with exact terms; the twin does not know about sweeps, and the same law written flat
    (depth 4) runs the wide sweeps: equal values term by term would need equal rounding, so the flat law is compared to 1e-14."""
    dim, kind, _ = SHAPES[shape]
    p, d = _case(shape, 1)
    terms = ["e[0]**2", "e[1]**2", "0.5*e[2]**2"] + [f"0.0625*abs(e[{k % 3}])" for k in range(8)]  # nothing the parser folds
    nested = terms[-1]
    for tm in reversed(terms[:-1]):
        nested = f"({tm} + {nested})"
    flat = " + ".join(terms)
    deep = _law(["c[0]", f"c[1]*(0.5 + 0.5/(1 + {nested}))"])
    wide = _law(["c[0]", f"c[1]*(0.5 + 0.5/(1 + {flat}))"])
    assert deep.depth == 16 and wide.depth <= 10
    kw = dict(max_iter=2, tol=1e-3, fields=True, return_coef=True, return_tangent_coef=True)
    got = _tangent(p, d, deep, shape, **kw)
    T, asym = deep.host_tangent(got.strain, got.coef, d["coef"], d["rows"][:, :3], d["points"])
    assert np.array_equal(got.tangent_coef, _stream(shape, T)) and np.array_equal(got.asymmetry, asym)
    other = _tangent(p, d, wide, shape, **kw)
    Tw, _ = wide.host_tangent(other.strain, other.coef, d["coef"], d["rows"][:, :3], d["points"])
    assert np.array_equal(other.tangent_coef, _stream(shape, Tw))
    assert np.abs(other.tangent_coef - got.tangent_coef).max() <= 1e-12 * np.abs(got.tangent_coef).max()


MATH = ("sin(e[0]) + cos(e[1] - e[2]) + tanh(e[2]) - exp(-(e[0]**2)) + 0.5*log(1 + e[1]**2) + sqrt(1 + e[2]**2) + max(-e[0], 0.25)"
        " + where(e[1] > 0, tan(0.25*tanh(e[1])), -e[1])")


@pytest.mark.parametrize("with_M", [0, 1])
def test_the_tangent_rules_of_the_math_opcodes_follow_the_twin(with_M):
    """SQRT SIN COS TAN EXP LOG TANH MAX SELECT NEG SUB in one law, mu = c1 (1 + 0.05 F(e)): their device tangent rules against
    ``host_tangent``.  The device's math functions and NumPy's differ by a few units in the last place (2 to 4 ulp, 1e-15, by the
    tables of the ROCm math library), each tangent rule multiplies one such value once, and F enters T with the factor 0.05 c1 |e|
    of order one: 1e-13 of the largest entry bounds a dozen such errors tenfold.  A wrong rule is off by order 1e-2."""
    p, d = _case("e2", with_M)
    law = _law(["c[0]", f"c[1]*(1 + 0.05*({MATH}))"])
    assert law.explicit
    got = _tangent(p, d, law, "e2", max_iter=2, tol=1e-3, fields=True, return_coef=True, return_tangent_coef=True)
    assert set(np.unique(got.status)) <= {0, 1}
    T, asym = law.host_tangent(got.strain, got.coef, d["coef"], d["rows"][:, :3], d["points"])
    want = _stream("e2", T)
    plain, _ = _law(["c[0]", "c[1]"]).host_tangent(got.strain, got.coef, d["coef"], d["rows"][:, :3], d["points"])
    part = np.abs(want - _stream("e2", plain)).max() / np.abs(want).max()  # what the derivative of F adds: the test looks at something
    dev = np.abs(got.tangent_coef - want).max() / np.abs(want).max()
    print(f"M={with_M}: |tangent_coef - twin| = {dev:.3e} of the largest entry; the law's derivative makes up {part:.2e} of it; "
          f"asymmetry {got.asymmetry.max():.3e} against {asym.max():.3e}")
    assert part > 1e-3
    assert dev <= 1e-13
    assert np.abs(got.asymmetry - asym).max() <= 1e-13


# -- 6. the macro Newton method --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["PoissonHMM", "LinearElasticityStratifiedHMM"])
def test_newton_reaches_the_secant_solution_in_fewer_steps(cls):
    from hommx_amd import fem, hmm, mesh

    macro, micro = lambda: mesh.create_unit_square(4, 4), lambda: mesh.create_unit_square(5, 5)
    if cls == "PoissonHMM":
        law, _ = TR.potential_law("poisson", 2)
        A = hmm.TwoPhase(lambda y: (y[0] - 0.5) ** 2 + (y[1] - 0.5) ** 2 < 0.09, lambda x: 10.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
        make = lambda: hmm.PoissonHMM(macro(), A, lambda x: 40.0 + 0.0 * x[0], micro(), 0.05)
    else:
        law, _ = TR.potential_law("elasticity", 2)
        A = hmm.TwoPhase(lambda y: y[0] < 0.5, lambda x: hmm.Lame(20.0 + 0.0 * x[0], 10.0 + 0.0 * x[0]),
                         lambda x: hmm.Lame(2.0 + 0.0 * x[0], 1.0 + 0.0 * x[0]))

        def make():
            h = hmm.LinearElasticityStratifiedHMM(macro(), A, lambda x: np.array([0.0, -8.0]), micro(), 0.05,
                                                  lambda x: np.array([[1.0, 0.1], [0.2, 0.9]]))
            V = h.function_space
            clamp = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1) | np.isclose(x[1], 0) | np.isclose(x[1], 1))
            h.set_boundary_conditions(fem.dirichletbc(fem.Function(V), clamp, V))
            return h

    hs, hn = make(), make()
    hn.prepare(newton=True)  # the sibling plan exists and is reserved with the plan before the first step, and is kept
    sibling = hn._tangent_plan
    assert sibling.kind == hn._plan.tangent_kind and hn._tangent_reserved == hn._reserved_cells == hn._msh.num_cells
    us = hs.solve_nonlinear(law, max_iter=80, tol=1e-11, micro_tol=1e-13, micro_iter=200).x.array.copy()
    un = hn.solve_nonlinear(law, max_iter=80, tol=1e-11, micro_tol=1e-13, micro_iter=200, method="newton").x.array.copy()
    dev = np.abs(un - us).max() / np.abs(us).max()
    print(f"{cls}: secant {len(hs.nonlinear_history)} steps, newton {len(hn.nonlinear_history)} steps, difference {dev:.2e} of max |u|; "
          f"newton history {['%.1e' % v for v in hn.nonlinear_history]}")
    assert dev <= 1e-8
    assert len(hn.nonlinear_history) < len(hs.nonlinear_history)
    assert hn.tangent_tensors.shape == hn.effective_tensors.shape and np.nanmax(hn.secant.asymmetry) <= 1e-12
    assert hn._tangent_plan is sibling and hs._tangent_plan is None
