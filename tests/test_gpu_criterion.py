"""Failure criteria on the reconstructed micro state, on the device (-m gpu; csrc/criterion.hip, hommx_criterion_source).

The shapes are those of test_gpu_elem_walk_bits.py, three seeded cells each, with and without M: every (DIM, KIND, MESH) class of
k_criterion.  What the device is held to is ``Criterion.host_values`` -- the NumPy interpreter of the same program -- fed with the strain,
the flux and the coefficient OF THE SAME CALL: a program of exactly rounded operations (+ - * /, sqrt, comparisons, where, min / max, abs)
must reproduce it bit for bit; a math function within the per-function rule of test_gpu_expr.py.  The call's own fields are compared with
``reconstruct(fields=True)`` (and, with a load, ``+ loads(...).flux[:, 0]``) to 1e-9 of the largest entry, what test_gpu_reconstruct.py
allows per-element fields: k_criterion forms them without contraction, k_recon with it.  The statistics must not depend on which outputs
are written, on the chunking, on the batch position or on the entry (host / device): bit for bit.
"""

import functools

import numpy as np
import pytest

from test_gpu_elem_walk_bits import NC, SHAPES, _inputs

pytestmark = pytest.mark.gpu

CASES = [(s, m) for s in SHAPES for m in (0, 1)]
# every exactly rounded opcode and every input class (x y p f e s c); indices 0 and 1 only, so it stands on every kind
EXACT = ("where((s[0] > e[0] and not c[0] < 0.5) or (y[0] <= x[1] and x[0] >= 0.25), abs(s[0] - e[1]) / (1 + c[0]**2), "
         "-min(s[1], e[0]*p[0])) + max(f[0], y[1])*sqrt(s[0]**2 + s[1]**2)")
MATH = {  # f -> its argument, built from exactly rounded operations of the state and bounded where f needs it
    "sqrt": "1 + s[0]**2",
    "sin": "0.25*s[0] + x[0]",
    "cos": "0.25*s[1] - y[0]",
    "tan": "0.125*min(max(s[0], -4), 4)",
    "exp": "0.25*min(s[0], 8)",
    "log": "1 + s[1]**2",
    "tanh": "0.5*e[0]",
}
MEASURED_ULP = {"sqrt": 0, "sin": 1, "cos": 1, "tan": 1, "exp": 1, "log": 1, "tanh": 1}  # test_gpu_expr.py; DESIGN section 3
NUMPY = {"sqrt": np.sqrt, "sin": np.sin, "cos": np.cos, "tan": np.tan, "exp": np.exp, "log": np.log, "tanh": np.tanh}


def _crit(text, **kw):
    from hommx_amd.expr import Criterion

    return Criterion(text, **kw)


def _deep():
    """A program of depth 16: fifteen pending left operands above the innermost value."""
    text = "c[0]"
    for i in range(15):
        text = f"(s[{i % 2}] {'+*'[i % 2]} {text})" if i % 3 else f"(e[{i % 2}] - {text})"
    crit = _crit(text, threshold=0.0)
    assert crit.depth == 16
    return crit


def _programs():
    flat = _crit("s[0]", threshold=0.0)
    assert flat.depth == 1
    return {"exact": _crit(EXACT, p=[0.75], fields=1, threshold=0.5), "deep": _deep(), "flat": flat}


@functools.lru_cache(maxsize=None)
def _plan_and_volumes(shape, load_solve=True):
    from hommx_amd import MicroCellPlan, workloads as W

    dim, kind, n = SHAPES[shape]
    if n:
        p = MicroCellPlan(dim, n, kind)
        return p, np.full(p.n_el, 1.0 / p.n_el)
    msh = W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)
    return MicroCellPlan.from_mesh(msh, kind, route="front", load_solve=load_solve), msh.cell_volumes()


@functools.lru_cache(maxsize=None)
def _case(shape, with_M):
    """The inputs of test_gpu_elem_walk_bits.py and, seeded, what a criterion reads beside them: rows (midpoint, one field) and points."""
    p, vol = _plan_and_volumes(shape)
    d = _inputs(p, shape, with_M)
    rng = np.random.default_rng(9100 + 10 * list(SHAPES).index(shape) + with_M)
    d["rows"] = rng.integers(-8, 9, (NC, 4)) / 8.0  # dyadic: the comparisons on x and f are decided alike on both sides
    d["points"] = rng.integers(0, 17, (p.n_el, p.dim)) / 16.0
    d["load"] = rng.standard_normal((NC, p.n_el, p.t))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p, vol, d


def _run(p, d, crit, **kw):
    rows = d["rows"][:, :3 + crit.n_fields]
    return p.criterion(d["coef"], d["xi"], crit, d["M"], rows=rows, points=d["points"], **kw)


def _at_median(p, d, crit, **kw):
    """`crit` with its threshold at the median of its values on this batch, so that the indicator splits the elements."""
    import copy

    out = copy.copy(crit)
    out.threshold = float(np.median(_run(p, d, crit, values=True, **kw).values))
    return out


def _host(crit, r, d):
    return crit.host_values(r.strain, r.flux, d["coef"], d["rows"][:, :3], d["points"], d["rows"][:, 3:3 + crit.n_fields])


def _stats(r):
    return np.stack([r.max, r.argmax_element.astype(float), r.mean, r.exceed_volume], axis=1)


def _check_statistics(r, crit, vol, what):
    """max / argmax bitwise from the values; mean and exceed_volume within the summation bound n_el 2^-52 sum |K| |v_K| of NumPy's sums."""
    v, n_el = r.values, r.values.shape[1]
    assert np.array_equal(r.max, v.max(axis=1)), what
    assert np.array_equal(r.argmax_element, np.argmax(v, axis=1)), what  # argmax: the first, i.e. the smallest, index reaching it
    over = (v >= crit.threshold).astype(float)
    for got, w in ((r.mean, v), (r.exceed_volume, over)):
        ref, bound = (vol * w).sum(axis=1), n_el * 2.0**-52 * (vol * np.abs(w)).sum(axis=1)
        print(f"{what}: |device - numpy| = {np.abs(got - ref).max():.3e}, bound {bound.min():.3e}")
        assert np.all(np.abs(got - ref) <= bound), what
    assert 0 < over.sum() < over.size, what  # the threshold splits the elements: the indicator is exercised


# -- 1. exactly rounded programs: the host twin bit for bit, the statistics from the values -------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_exact_programs_equal_the_host_twin_bitwise(shape, with_M):
    p, vol, d = _case(shape, with_M)
    for name, crit in _programs().items():
        crit = _at_median(p, d, crit)
        r = _run(p, d, crit, values=True, fields=True)
        assert not r.info.any()
        assert np.array_equal(r.values, _host(crit, r, d)), name
        _check_statistics(r, crit, vol, f"{shape} M{with_M} {name}")
        for kw in ({}, {"values": True}, {"fields": True}):  # the statistics do not depend on OUT
            assert np.array_equal(_stats(_run(p, d, crit, **kw)), _stats(r)), (name, kw)


# -- 2. math functions: the per-function rule of test_gpu_expr.py -------------------------------------------------------------------------
@pytest.mark.parametrize("f", list(MATH))
@pytest.mark.parametrize("shape", ["p2", "e3", "mesh_p2"])
def test_math_functions_within_their_ulps(shape, f):
    p, vol, d = _case(shape, 0)
    c0, c1 = 0.25, 1.5
    crit = _crit(f"{c0} + {c1}*{f}({MATH[f]})")
    r = _run(p, d, crit, values=True, fields=True)
    host = _host(crit, r, d)
    arg = _host(_crit(MATH[f]), r, d)
    fmax = np.abs(NUMPY[f](arg)).max()
    U = max(2, 2 * MEASURED_ULP[f])
    tol = abs(c1) * (U + 1) * 2.0**-52 * fmax
    err = np.abs(r.values - host).max()
    print(f"{shape} {f}: max |device - host| = {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert np.array_equal(r.max, r.values.max(axis=1))


# -- 3. the call's own fields against the existing calls; flux_norm against max_flux ----------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_fields_and_flux_norm_match_reconstruct(shape, with_M):
    from hommx_amd.expr import Criterion

    p, vol, d = _case(shape, with_M)
    crit = Criterion.flux_norm(p.kind, p.dim)
    r = _run(p, d, crit, values=True, fields=True)
    ref = p.reconstruct(d["coef"], d["xi"], d["M"], fields=True)
    for name in ("strain", "flux"):
        got, want = getattr(r, name), getattr(ref, name)
        dev = np.abs(got - want).max() / np.abs(want).max()
        print(f"{shape} M{with_M} {name}: deviation from reconstruct {dev:.3e} of the largest entry")
        assert dev <= 1e-9
    assert np.array_equal(r.A_eff, ref.A_eff)
    assert np.allclose(r.max, ref.max_flux, rtol=1e-10, atol=0)
    top = np.sort(r.values, axis=1)[:, -2:]
    clear = top[:, 1] - top[:, 0] > 1e-10 * top[:, 1]
    assert clear.any()
    assert np.array_equal(r.argmax_element[clear], ref.argmax_element[clear])


# -- 4. bitwise independence: chunking, batch position, entry ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2", "e3", "mesh_p2"])
def test_statistics_do_not_depend_on_chunking_or_batch_position(shape, monkeypatch):
    p, vol, d = _case(shape, 1)
    crit = _programs()["exact"]
    want = _stats(_run(p, d, crit))
    one = p.criterion(d["coef"][1:2], d["xi"][1:2], crit, d["M"][1:2], rows=d["rows"][1:2], points=d["points"])
    assert np.array_equal(_stats(one)[0], want[1])
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")
    _plan_and_volumes.cache_clear()  # the variable is read when a plan is created
    try:
        q, _ = _plan_and_volumes(shape)
        per_cell = ("coef", "M", "xi", "rows")
        big = {k: (np.concatenate([v] * 120) if k in per_cell else v) for k, v in d.items()}
        got = _stats(_run(q, big, crit))  # 360 cells: at least two chunks of 1 MB of correctors (3.9 KiB per cell at the smallest shape)
        assert np.array_equal(got, np.concatenate([want] * 120))
        q.close()
    finally:
        _plan_and_volumes.cache_clear()
        _case.cache_clear()


@pytest.mark.parametrize("shape,load", [("p2", False), ("e2", True), ("mesh_ev3", False)])
def test_device_entry_equals_host_entry(shape, load):
    import torch

    from hommx_amd.batch import CoefStream

    p, vol, d = _case(shape, 1)
    crit = _programs()["exact"]
    P = d["load"] if load else None
    want = p.criterion(d["coef"], d["xi"], crit, d["M"], rows=d["rows"], points=d["points"], values=True, fields=True, P=P)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    out = {"crit": empty(NC, 4), "values": empty(NC, p.n_el), "strain": empty(NC, p.n_el, p.t), "flux": empty(NC, p.n_el, p.t),
           "A_eff": empty(NC, p.t, p.t), "info": empty(NC, dtype=torch.int32)}
    p.criterion_device(NC, CoefStream.sampled(d["coef"]).coef_source(upload), upload(d["M"]), upload(d["xi"]), crit, upload(d["rows"]),
                       out["crit"].data_ptr(), upload(d["points"]), out["values"].data_ptr(), out["strain"].data_ptr(), out["flux"].data_ptr(),
                       P_ptr=upload(P) if load else None, A_ptr=out["A_eff"].data_ptr(), info_ptr=out["info"].data_ptr(),
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["crit"], _stats(want))
    for k in ("values", "strain", "flux", "A_eff", "info"):
        assert np.array_equal(got[k], getattr(want, k)), k


# -- 5. loads: the total state, three ways to supply the load -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2", "e3", "mesh_p2"])
@pytest.mark.parametrize("how", ["array", "eigenstrain", "program"])
def test_with_a_load_the_criterion_sees_the_total_state(shape, how):
    from hommx_amd.batch import CoefStream
    from hommx_amd.expr import Expression

    p, vol, d = _case(shape, 1)
    crit = _programs()["exact"]
    assert p.load_kernel == {"p2": "fused2d_subst", "e3": "blocked", "mesh_p2": "mesh_front_subst"}[shape]
    if how == "program":  # a vector Expression of the load's own, sampled at the centroids with weight 1
        E = Expression([f"{k + 1}*y[0] - x[1] + f[0]*y[{k % p.dim}]" for k in range(p.t)], fields=1)
        P = CoefStream.program(d["points"][:, None, :], np.ones(1), *E.program(), p.t, d["rows"], n_fields=1)
        kw = {}
    else:
        P, kw = d["load"], ({"eigenstrain": True} if how == "eigenstrain" else {})
    crit = _at_median(p, d, crit, P=P, **kw)
    r = p.criterion(d["coef"], d["xi"], crit, d["M"], rows=d["rows"], points=d["points"], values=True, fields=True, P=P, **kw)
    assert np.array_equal(r.values, _host(crit, r, d))
    _check_statistics(r, crit, vol, f"{shape} {how}")
    ref = p.reconstruct(d["coef"], d["xi"], d["M"], fields=True)
    lr = p.loads(d["coef"], P if how == "program" else P[:, None], d["M"], fields=True, **kw)
    for name in ("strain", "flux"):
        want = getattr(ref, name) + getattr(lr, name)[:, 0]
        dev = np.abs(getattr(r, name) - want).max() / np.abs(want).max()
        print(f"{shape} {how} {name}: deviation from reconstruct + loads {dev:.3e} of the largest entry")
        assert dev <= 1e-9
    assert np.array_equal(_stats(p.criterion(d["coef"], d["xi"], crit, d["M"], rows=d["rows"], points=d["points"], P=P, **kw)), _stats(r))


def test_frontal_mesh_plan_without_a_load_solve_refuses_a_load():
    from hommx_amd._lib import HommxLibraryError

    p, vol, d = _case("mesh_p2", 0)
    q, _ = _plan_and_volumes("mesh_p2", False)
    crit = _programs()["flat"]
    assert np.array_equal(_stats(_run(q, d, crit)), _stats(_run(p, d, crit)))  # without a load it serves the criterion
    with pytest.raises(HommxLibraryError, match="frontal mesh route"):
        _run(q, d, crit, P=d["load"])


# -- 6. bad input cells ----------------------------------------------------------------------------------------------------------------------
def test_a_nan_cell_leaves_the_others_alone_and_a_nan_value_never_wins():
    p, vol, d = _case("e2", 1)
    crit = _programs()["exact"]
    want = _stats(_run(p, d, crit))
    bad = dict(d, coef=d["coef"].copy())
    bad["coef"][1, 7, 0] = np.nan
    r = _run(p, bad, crit)
    assert r.info[1] > 0 and not r.info[[0, 2]].any()
    assert np.array_equal(_stats(r)[[0, 2]], want[[0, 2]])
    # a criterion that is NaN on some elements (the root of a negative: those whose centroid has y[0] < 0.5 -- the sign of s[0] follows
    # the macro strain and would make whole cells NaN): the mean says so, the maximum is that of the rest
    root = _crit("sqrt(y[0] - 0.5) + abs(s[0])", threshold=0.0)
    r = _run(p, d, root, values=True)
    nan = np.isnan(r.values)
    assert nan.any(axis=1).all() and not nan.all(axis=1).any()
    assert np.isnan(r.mean).all()
    assert np.array_equal(r.max, np.nanmax(r.values, axis=1))
    assert np.array_equal(r.argmax_element, np.nanargmax(r.values, axis=1))
    over = (vol * (r.values >= 0.0)).sum(axis=1)  # a NaN value is not above the threshold
    assert np.all(np.abs(r.exceed_volume - over) <= r.values.shape[1] * 2.0**-52 * over)


# -- 7. the slot path: a field that does not fit LDS beside the stack -----------------------------------------------------------------------
def test_slot_path_and_lds_path_on_a_large_cell():
    from hommx_amd import MicroCellPlan

    n, nc = 112, 2  # 8 ndof = 98 KiB: with the 60 KiB of fifteen stack rows above the 150 KiB limit of the reconstruction, with one row below it
    p = MicroCellPlan(2, n, "poisson")
    rng = np.random.default_rng(11)
    d = {"coef": np.exp(rng.uniform(-1, 1, (nc, p.n_el))), "xi": rng.standard_normal((nc, 2)), "M": None,
         "rows": rng.integers(-8, 9, (nc, 4)) / 8.0, "points": rng.integers(0, 17, (p.n_el, 2)) / 16.0}
    vol = np.full(p.n_el, 1.0 / p.n_el)
    shallow = _crit("s[0]*e[1] - c[0]", threshold=0.0)
    assert shallow.depth == 2 and 8 * n * n + 4096 * 15 > 150 * 1024 >= 8 * n * n + 4096
    for name, crit in (("slot", _deep()), ("lds", shallow)):
        crit = _at_median(p, d, crit)
        r = _run(p, d, crit, values=True, fields=True)
        assert not r.info.any()
        assert np.array_equal(r.values, _host(crit, r, d)), name
        _check_statistics(r, crit, vol, name)
        assert np.array_equal(_stats(_run(p, d, crit)), _stats(r)), name
    p.close()


# -- 8. the solver classes ----------------------------------------------------------------------------------------------------------------------
def test_linear_elasticity_hmm_end_to_end():
    """h.criterion() against host_values of reconstruct(fields=True) + load_response(fields=True).  The criterion is a polynomial,
    v = (s0^2 - s0 s1 + s1^2 + 3 s2^2) / strength(c)^2 with strength 900 or 60: for fields within delta = 1e-9 S of each other, S the
    largest |s| entry, |dv| <= (|dv/ds0| + |dv/ds1| + |dv/ds2|) delta + O(delta^2) <= (3 S + 3 S + 6 S) delta / 60^2 -- the bound
    asserted, with a factor 2 for the second order and the rounding of the evaluation itself."""
    from hommx_amd import hmm, mesh
    from hommx_amd.expr import Criterion, Expression

    A = hmm.TwoPhase(lambda y: (y[0] - 0.5) ** 2 + (y[1] - 0.5) ** 2 < 0.09, lambda x: hmm.Lame(60.0 + 0.0 * x[0], 40.0 + 10.0 * x[0]),
                     lambda x: hmm.Lame(2.0 + 0.0 * x[0], 1.0 + 0.0 * x[0]))
    h = hmm.LinearElasticityHMM(mesh.create_unit_square(8, 8), A, lambda x: np.array([0.0, -1.0]), mesh.create_unit_square(8, 8), 0.05)
    h.set_eigenstrain(Expression(["1e-3*f[0]", "1e-3*f[0]*(1 + y[0])", "0"], fields=1))
    h.set_polarisation_fields(lambda x: 1.0 + x[0])
    x = h.function_space.tabulate_dof_coordinates()[:, :2]
    u = np.stack([0.01 * x[:, 0] * x[:, 1], -0.02 * x[:, 1] ** 2], axis=1).ravel()
    crit = Criterion("(s[0]**2 - s[0]*s[1] + s[1]**2 + 3*s[2]**2) / where(c[1] > 20, 900, 60)**2", threshold=1e-9)
    r = h.criterion(crit, u, values=True, chunk_cells=50)
    rec, lr = h.reconstruct(u, fields=True), h.load_response(fields=True)
    strain, flux = rec.strain + lr.strain[:, 0], rec.flux + lr.flux[:, 0]
    stream, kind = h._coef_stream(r.cells)
    coef = stream.per_cell if stream.method == "solve" else h._ensure_plan(kind).expand(stream)  # what the device read as c
    want = crit.host_values(strain, flux, coef, np.zeros((len(r.cells), 3)))
    S = np.abs(flux).max()
    bound = 2 * 12 * S * (1e-9 * S) / 60.0**2
    err = np.abs(r.values - want).max()
    print(f"h.criterion against host_values of reconstruct + load_response: {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(r.max, r.values.max(axis=1)) and r.exceed_volume.min() >= 0 and r.exceed_volume.max() <= 1 + 1e-12
    mech = h.criterion(crit, u, load=False, values=True)
    assert np.abs(mech.values - crit.host_values(rec.strain, rec.flux, coef, np.zeros((len(r.cells), 3)))).max() <= bound
    assert not np.array_equal(mech.values, r.values)
