"""History variables of a strain-dependent law on the device (-m gpu; k_secant_history of csrc/secant.hip, k_secant_tangent_history of
csrc/secant_tangent.hip, hommx_secant_history_source, hommx_secant_tangent_history_source), on the six shapes of
test_gpu_elem_walk_bits.py, three seeded cells each: every (DIM, KIND, MESH) class of the two kernels.  Held:

a. the law and the updates bit for bit: ``host_values(history=)`` / ``host_history`` fed with the strain, the flux, the base coefficient
   and the history of the same call reproduce ``values`` and ``history`` for a program of exactly rounded operations that reads
   x y p f e s c h, with four history variables on ``p2`` and one elsewhere;
b. a law whose components ignore ``h`` has the bits of ``secant()`` with the plain law in every shared output;
c. load / unload / reload against tests/history_ref.py on ``p2`` and ``e2``: rounds within one, ``A_eff`` and ``history`` to 1e-9 of the
   largest entry (the bound of test_gpu_secant.py); unloading stops in 2 rounds with the history's bits and the linear response of
   the damaged stream;
d. no bit of ``history`` depends on the chunking, the batch position, ``max_iter`` beyond the stopping round, the outputs asked for or
   the entry;
e. a cell of status 2 or 3 keeps the bits of its input history and leaves the others alone;
f. the tangent: ``tangent_coef`` and ``asymmetry`` are ``host_tangent(history=)`` bit for bit, ``tangent`` is the sibling plan's solve, D
   against central differences of the reference's ``mean_flux`` at frozen history to 1e-8, tangent = A_eff under unloading;
g. the slot path of a large cell; h. the solver classes end to end.

The damage law scales every entry of the base coefficient by g(kappa) = 1 - 0.5 (1 - exp(-kappa / 0.7)), kappa = max(h0, |e|) with
|e| = sqrt(e0^2 + e1^2): s -> s g(s) is increasing (its derivative is at least 0.43), so the iteration converges, and g lies in
(0.5, 1], so the tensor stays a positive multiple of the base.
"""

import functools

import numpy as np
import pytest

import history_ref as HR
from test_gpu_elem_walk_bits import NC, SHAPES
from test_gpu_secant import CASES, N_COMP, _bits, _case, _check_consistent, _law, _plan, _solver, soft_law
from test_gpu_secant_tangent import _sibling, _stream

pytestmark = pytest.mark.gpu

EQ = "sqrt(e[0]**2 + e[1]**2)"
KAPPA = f"max(h[0], {EQ})"
G = f"(1 - 0.5*(1 - exp(-{KAPPA}/0.7)))"


def damage_law(kind, dim, scale="", extra="", **kw):
    """Every entry of the base coefficient times g(kappa) (module docstring); ``scale``: a text in front of every component,
    ``extra``: one behind it."""
    n = N_COMP[kind](dim)
    assert n <= 6
    return _law([f"{scale}c[{k}]*{G}{extra}" for k in range(n)], matrix=kind == "poisson_matrix", history=[KAPPA], history_names=("kappa",), **kw)


def potential_damage_law(kind, dim):
    """A damage law with a potential, for the comparison of D with differences: the stress is g(kappa) C e, and its derivative is
    symmetric when kappa is driven by the energy norm sqrt(e . C e) of the BASE tensor -- |e| times sqrt(c) for scalar Poisson (|e|
    serves as well: C is a multiple of the identity), lam tr(e)^2 + 2 mu (e0^2 + e1^2) + mu e2^2 for 2D Lame."""
    if kind == "poisson":
        return damage_law(kind, dim)
    assert kind == "elasticity" and dim == 2
    kappa = "max(h[0], sqrt(c[0]*(e[0] + e[1])**2 + 2*c[1]*(e[0]**2 + e[1]**2) + c[1]*e[2]**2))"
    g = f"(1 - 0.5*(1 - exp(-{kappa}/0.7)))"
    return _law([f"c[0]*{g}", f"c[1]*{g}"], history=[kappa], history_names=("kappa",))


def exact_law(kind, dim, n_history):
    """Exactly rounded operations only (+ - * / abs min max sqrt, comparisons, where), reading x y p f e s c h.  Component 0 reads all
    of them, components 1 .. 5 one product of the state and one of the history, the Voigt entries from 6 on are copies.  The updates:
    a running maximum; with four variables also a sum, a minimum and a choice."""
    n = N_COMP[kind](dim)
    first = ("where(s[0] > e[0] or y[0] <= x[1], abs(s[0] - e[1]) / (1 + c[0]**2), -min(s[1], e[0]*p[0])) + "
             "max(f[0], h[0])*sqrt(s[0]**2 + s[1]**2)")
    rest = [f"c[{k}]*s[{k % 2}] - e[{(k + 1) % 2}]*h[{k % n_history}]" if k < 6 else f"c[{k}]" for k in range(1, n)]
    updates = ["max(h[0], abs(e[0]) + y[1]*s[1])", "h[1] + 0.5*(s[1] - h[0])*c[0]", "min(h[2], e[1]*x[0] - f[0])",
               "where(h[3] > e[0], h[3], e[0]/p[0])"][:n_history]
    return _law([first] + rest, p=[0.75], fields=1, matrix=kind == "poisson_matrix", history=updates)


def exact_explicit_law(kind, dim):
    """The same for the tangent: no s; the first component softens with the larger of h0 and |e0| -- both branches of max occur --,
    the others with one strain entry and the history; of the 21 Voigt entries the fifteen off the diagonal are copies."""
    import secant_tangent_ref as TR

    t, n = TR.tensor_size(kind, dim), N_COMP[kind](dim)
    first = "c[0]*(p[0] + 0.25/(1 + max(h[0], abs(e[0])) + f[0]**2*abs(e[1]) + abs(x[0])*y[0]*y[1]))"
    diagonal = {k for k, (r, c) in enumerate(TR.entries(kind, dim)) if r == c} if kind == "elasticity_voigt" else set(range(n))
    more = " + h[0]" if n <= 6 else ""  # the 128 instructions do not hold it six times beside the 21 stores
    rest = [f"c[{k}]*(1 + 0.25/(1 + e[{k % t}]**2{more}))" if k in diagonal else f"c[{k}]" for k in range(1, n)]
    return _law([first] + rest, p=[0.75], fields=1, matrix=kind == "poisson_matrix", history=["max(h[0], abs(e[0]))"])


def _history(shape, with_M, n_history=1, scale=1.0):
    """A seeded dyadic history in [0, 2) * scale: some elements of a cell will load, some will not."""
    p = _plan(shape)
    rng = np.random.default_rng(9700 + 10 * list(SHAPES).index(shape) + with_M)
    h = scale * rng.integers(0, 16, (NC, p.n_el, n_history)) / 8.0
    h.setflags(write=False)
    return h


def _run(p, d, law, history, **kw):
    rows = d["rows"][:, :3 + law.n_fields]
    return p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, points=d["points"], history=history, **kw)


def _tangent(p, d, law, shape, history, **kw):
    rows = d["rows"][:, :3 + law.n_fields]
    return p.secant_tangent(d["coef"], d["xi"], law, _sibling(shape), d["M"], rows=rows, points=d["points"], history=history, **kw)


def _hbits(r):
    return _bits(r) + [r.history]


def _same(a, b, cells=slice(None), what=""):
    for x, y in zip(_hbits(a), _hbits(b)):
        if x is not None and y is not None:
            assert np.array_equal(x[cells], y[cells], equal_nan=x.dtype.kind == "f"), what


# -- a. the twins, bit for bit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_exact_program_equals_the_host_twins_bitwise(shape, with_M):
    p, d = _case(shape, with_M)
    nh = 4 if shape == "p2" else 1
    law, h = exact_law(p.kind, p.dim, nh), _history(shape, with_M, nh)
    r = _run(p, d, law, h, max_iter=1, fields=True, values=True, return_coef=True)
    assert not r.info.any() and np.array_equal(r.rounds, np.ones(NC, dtype=np.int64)) and set(np.unique(r.status)) <= {0, 1}
    args = (r.strain, r.flux, d["coef"], d["rows"][:, :3], d["points"], d["rows"][:, 3:4])
    assert r.values.shape == (NC, p.n_el, p.n_comp) and r.history.shape == (NC, p.n_el, nh)
    assert np.array_equal(r.values, law.host_values(*args, history=h))
    assert np.array_equal(r.history, law.host_history(*args, history=h))
    assert not np.array_equal(r.history, h)  # the updates do something
    assert np.array_equal(r.coef, d["coef"])  # a stopping round commits nothing
    again = _run(p, d, law, h[:, :, 0] if nh == 1 else h, max_iter=1)  # [N, n_el] for one variable; no optional output
    assert np.array_equal(again.history, r.history) and np.array_equal(again.A_eff, r.A_eff)


# -- b. a law that does not read its history ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_a_history_blind_law_has_the_bits_of_the_plain_law(shape, with_M):
    p, d = _case(shape, with_M)
    plain = soft_law(p.kind, p.dim)
    blind = _law(list(plain.texts), matrix=p.kind == "poisson_matrix", history=["max(h[0], abs(e[0]))"])
    h = _history(shape, with_M, scale=0.25)
    kw = dict(max_iter=5, tol=1e-3, fields=True, return_coef=True)
    want = p.secant(d["coef"], d["xi"], plain, d["M"], rows=d["rows"][:, :3], points=d["points"], **kw)
    got = _run(p, d, blind, h, **kw)
    for x, y in zip(_bits(got) + [got.strain, got.flux], _bits(want) + [want.strain, want.flux]):
        assert np.array_equal(x, y)
    assert len(set(got.rounds.tolist()) | {0}) >= 2 and not got.info.any()
    twin = blind.host_history(got.strain, got.flux, d["coef"], d["rows"][:, :3], d["points"], history=h)
    assert np.array_equal(got.history, twin) and np.array_equal(twin[:, :, 0], np.maximum(h[:, :, 0], np.abs(got.strain[:, :, 0])))


# -- c. load, unload, reload against the reference ------------------------------------------------------------------------------------------
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _reference_path(shape):
    """history_ref on the three cells of `shape` with M along xi, xi / 2, 1.5 xi, each step from the history of the step before:
    computed once, read only."""
    p, d = _case(shape, 1)
    law, solve = damage_law(p.kind, p.dim), _solver(shape)
    steps, h = [], np.zeros((NC, p.n_el, 1))
    for scale in (1.0, 0.5, 1.5):
        rs = [HR.iterate(solve, law, d["coef"][c], scale * d["xi"][c], h[c], d["M"][c], d["rows"][c, :3], d["points"], max_iter=100, tol=TOL)
              for c in range(NC)]
        h = np.stack([r["history"] for r in rs])
        steps.append(rs)
    return steps


@pytest.mark.parametrize("shape", ["p2", "e2"])
def test_load_unload_reload_against_the_reference(shape):
    p, d = _case(shape, 1)
    law, ref = damage_law(p.kind, p.dim), _reference_path(shape)
    h = np.zeros((NC, p.n_el, 1))
    for step, scale in enumerate((1.0, 0.5, 1.5)):
        dd = dict(d, xi=scale * d["xi"])
        r = _run(p, dd, law, h, max_iter=100, tol=TOL, return_coef=True)
        want = ref[step]
        rounds = [x["rounds"] for x in want]
        print(f"{shape} step {step} (scale {scale}): rounds {r.rounds.tolist()} against {rounds} of the reference")
        assert all(x["status"] == 0 for x in want) and not r.status.any() and not r.info.any()
        assert np.all(np.abs(r.rounds - np.array(rounds)) <= 1)
        for c in range(NC):
            dA = np.abs(r.A_eff[c] - want[c]["A"]).max() / np.abs(want[c]["A"]).max()
            dh = np.abs(r.history[c] - want[c]["history"]).max() / np.abs(want[c]["history"]).max()
            print(f"  cell {c}: A_eff {dA:.3e}, history {dh:.3e} (relative to the largest entry)")
            assert dA <= 1e-9 and dh <= 1e-9
        _check_consistent(p, dd, r, f"{shape} step {step}")
        if step == 0:
            assert (r.history > 0).all()
        if step == 1:  # unloading
            assert np.array_equal(r.rounds, np.full(NC, 2)) and rounds == [2] * NC
            assert np.array_equal(r.history, h)  # not a bit
            A = p.solve(r.coef, d["M"])  # the damaged stream: the response is its linear one
            assert np.abs(A - r.A_eff).max() <= 1e-12 * np.abs(A).max()
        if step == 2:
            assert (r.history > h).all()
        h = r.history


# -- d. what no bit of the history depends on -------------------------------------------------------------------------------------------------
def _staggered(shape):
    """The batch of `shape` with M, its macro strains scaled by 0.1, 1 and 3 and a history in between: cell 0 unloads, the cells stop
    in different rounds."""
    p, d = _case(shape, 1)
    return p, dict(d, xi=d["xi"] * np.array([0.1, 1.0, 3.0])[:, None]), _history(shape, 1, scale=0.5)


@pytest.mark.parametrize("shape", ["p2", "mesh_p2"])
def test_a_frozen_cell_keeps_its_history_whatever_happens_around_it(shape, monkeypatch):
    p, d, h = _staggered(shape)
    law = damage_law(p.kind, p.dim)
    want = _run(p, d, law, h, max_iter=60, return_coef=True)
    print(f"{shape}: rounds {want.rounds.tolist()}")
    assert not want.status.any() and len(set(want.rounds.tolist())) > 1
    twin = _run(p, d, law, h, max_iter=60, return_coef=True, fields=True, values=True)
    _same(twin, want, what="outputs")
    assert np.array_equal(twin.history, law.host_history(twin.strain, twin.flux, d["coef"], d["rows"][:, :3], d["points"], history=h))
    _same(_run(p, d, law, h, max_iter=60), want, what="no optional output")
    early = want.rounds < 25
    assert early.any()
    _same(_run(p, d, law, h, max_iter=25, return_coef=True), want, early, "max_iter")
    order = [2, 0, 1]
    swapped = p.secant(d["coef"][order], d["xi"][order], law, d["M"][order], rows=d["rows"][order, :3], points=d["points"], max_iter=60,
                       return_coef=True, history=h[order])
    for x, y in zip(_hbits(swapped), _hbits(want)):
        assert np.array_equal(x, y[order])
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")
    _plan.cache_clear()  # the variable is read when a plan is created
    try:
        q = _plan(shape)
        rep = 120  # 360 cells: at least two chunks of 1 MB of correctors (3.9 KiB per cell at the smallest shape)
        tile = lambda a: np.concatenate([a] * rep)
        got = q.secant(tile(d["coef"]), tile(d["xi"]), law, tile(d["M"]), rows=tile(d["rows"][:, :3]), points=d["points"], max_iter=60,
                       return_coef=True, history=tile(h))
        for x, y in zip(_hbits(got), _hbits(want)):
            assert np.array_equal(x, tile(y))
        q.close()
    finally:
        _plan.cache_clear()
        _case.cache_clear()


@pytest.mark.parametrize("shape", ["p2", "e2"])
def test_device_entries_equal_host_entries(shape):
    import torch

    from hommx_amd.batch import CoefStream

    p, d, h = _staggered(shape)
    law = damage_law(p.kind, p.dim)
    want = _tangent(p, d, law, shape, h, max_iter=60, return_coef=True, return_tangent_coef=True)
    assert np.array_equal(want.history, _run(p, d, law, h, max_iter=60).history)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    for tangent in (False, True):
        out = {"state": empty(NC, 3), "A_eff": empty(NC, p.t, p.t), "mean_flux": empty(NC, p.t), "coef": empty(*d["coef"].shape),
               "info": empty(NC, dtype=torch.int32), "history": empty(NC, p.n_el, 1), "tangent": empty(NC, p.t, p.t), "asymmetry": empty(NC),
               "tangent_coef": empty(NC, p.n_el, p.t * (p.t + 1) // 2)}
        ptr = {k: v.data_ptr() for k, v in out.items()}
        common = dict(points_ptr=upload(d["points"]), max_iter=60, mean_flux_ptr=ptr["mean_flux"], coef_ptr=ptr["coef"], info_ptr=ptr["info"],
                      stream=torch.cuda.current_stream(dev).cuda_stream, history_in_ptr=upload(h), history_out_ptr=ptr["history"])
        source = CoefStream.sampled(d["coef"]).coef_source(upload)
        if tangent:
            p.secant_tangent_device(NC, source, upload(d["M"]), upload(d["xi"]), law, _sibling(shape), upload(d["rows"][:, :3]), ptr["state"],
                                    ptr["A_eff"], ptr["tangent"], ptr["asymmetry"], tangent_coef_ptr=ptr["tangent_coef"], **common)
        else:
            p.secant_device(NC, source, upload(d["M"]), upload(d["xi"]), law, upload(d["rows"][:, :3]), ptr["state"], ptr["A_eff"], **common)
        torch.cuda.synchronize(dev)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert np.array_equal(got["state"], np.stack([want.rounds, want.change, want.status], axis=1).astype(np.float64))
        for k in ("A_eff", "mean_flux", "coef", "info", "history") + (("tangent", "asymmetry", "tangent_coef") if tangent else ()):
            assert np.array_equal(got[k], getattr(want, k)), (tangent, k)
    with pytest.raises(ValueError, match="history_in_ptr and history_out_ptr"):
        p.secant_device(NC, None, None, 0, law, 0, 0, 0)
    with pytest.raises(ValueError, match="two different device arrays"):
        p.secant_device(NC, None, None, 0, law, 0, 0, 0, history_in_ptr=ptr["history"], history_out_ptr=ptr["history"])


def test_the_plan_names_the_shape_it_expects():
    p, d = _case("p2", 1)
    law = damage_law(p.kind, p.dim)
    with pytest.raises(ValueError, match=rf"the law has the history variables kappa: pass history\[N_c, n_el, n_history\] = \({NC}, {p.n_el}, 1\)"):
        p.secant(d["coef"], d["xi"], law, d["M"])
    with pytest.raises(ValueError, match=r"history has shape \(3, 5, 1\); expected history\[N_c, n_el, n_history\]"):
        p.secant(d["coef"], d["xi"], law, d["M"], history=np.zeros((NC, 5, 1)))
    with pytest.raises(ValueError, match="no history variables"):
        p.secant(d["coef"], d["xi"], soft_law(p.kind, p.dim), d["M"], history=0.0)
    r = p.secant(d["coef"], d["xi"], law, d["M"], history=0.0, max_iter=1)  # a scalar: the initial state of every element
    assert np.array_equal(r.history, _run(p, d, law, np.zeros((NC, p.n_el, 1)), max_iter=1).history)


# -- e. the cells that fail -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["component", "update"])
@pytest.mark.parametrize("shape", ["p2", "e2"])
def test_a_value_that_is_not_finite_keeps_the_history_of_its_cell(shape, where):
    p, d, h = _staggered(shape)
    bad = " + 1e-300/(f[0] - 1)"
    if where == "component":
        law = damage_law(p.kind, p.dim, extra=bad, fields=1)
    else:
        law = _law(list(damage_law(p.kind, p.dim).texts), matrix=False, history=[KAPPA + bad], fields=1)
    rows = np.concatenate([d["rows"][:, :3], np.zeros((NC, 1))], axis=1)
    run = lambda: p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, points=d["points"], max_iter=60, return_coef=True, history=h)
    want = run()
    assert not want.status.any() and not np.array_equal(want.history[1], h[1])
    rows[1, 3] = 1.0
    r = run()
    assert r.status.tolist() == [0, 2, 0] and r.rounds[1] == 1
    assert np.array_equal(r.history[1], h[1]) and np.array_equal(r.coef[1], d["coef"][1])
    _same(r, want, [0, 2], "the other cells")


@pytest.mark.parametrize("shape", ["p2", "e2"])
def test_a_flagged_pivot_keeps_the_history_of_its_cell(shape):
    p, d, h = _staggered(shape)
    law = damage_law(p.kind, p.dim, scale="f[0]*", fields=1)
    rows = np.concatenate([d["rows"][:, :3], np.ones((NC, 1))], axis=1)
    run = lambda: p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, points=d["points"], max_iter=60, return_coef=True, history=h)
    want = run()
    assert not want.status.any()
    rows[1, 3] = -1.0
    r = run()
    assert r.status.tolist() == [0, 3, 0] and r.info[1] != 0 and not r.info[[0, 2]].any()
    assert r.rounds[1] == 2  # round 1 wrote its updates; the round that met the flagged pivot put the input back
    assert np.array_equal(r.history[1], h[1])
    _same(r, want, [0, 2], "the other cells")


# -- f. the tangent ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", CASES)
def test_tangent_coefficient_is_the_twins_and_shared_outputs_those_of_secant(shape, with_M):
    p, d = _case(shape, with_M)
    law, h = exact_explicit_law(p.kind, p.dim), _history(shape, with_M, scale=0.5)
    kw = dict(max_iter=3, tol=1e-3, fields=True, values=True, return_coef=True)
    want = _run(p, d, law, h, **kw)
    got = _tangent(p, d, law, shape, h, return_tangent_coef=True, **kw)
    for name in ("A_eff", "mean_flux", "rounds", "change", "status", "info", "coef", "strain", "flux", "values", "history"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert set(np.unique(got.status)) <= {0, 1}
    loads = np.abs(got.strain[:, :, 0]) > h[:, :, 0]
    assert loads.any() and not loads.all()  # both branches of max
    T, asym = law.host_tangent(got.strain, got.coef, d["coef"], d["rows"][:, :3], d["points"], d["rows"][:, 3:4], history=h)
    assert np.array_equal(got.tangent_coef, _stream(shape, T)), "tangent_coef"
    assert np.array_equal(got.asymmetry, asym), "asymmetry"
    D, info = _sibling(shape).solve(got.tangent_coef, d["M"], return_info=True)
    assert np.array_equal(info, got.tangent_info) and not info.any()
    assert np.array_equal(D, got.tangent)


@pytest.mark.parametrize("shape", ["p2", "e2"])
def test_tangent_against_central_differences_of_the_reference_at_frozen_history(shape):
    """A law with a potential (D is then the derivative itself, not that of a symmetrised law).  The history: what a loading step at xi
    left, halved on the elements of even index and times 1.5 on the odd ones, so at xi half of the elements load and half unload, none
    near the kink.  D of the device against (mean_flux(xi + d) - mean_flux(xi - d)) / 2 d of history_ref.iterate at that history, on
    the CPU: d = 1e-5, tol = 1e-14; 1e-8 of the largest entry, the bound of test_secant_tangent_host.py."""
    p, d = _case(shape, 1)
    law, solve = potential_damage_law(p.kind, p.dim), _solver(shape)
    loaded = _run(p, d, law, 0.0, max_iter=200, tol=1e-12)
    assert not loaded.status.any()
    h = loaded.history * np.where(np.arange(p.n_el) % 2 == 0, 0.5, 1.5)[None, :, None]
    got = _tangent(p, d, law, shape, h, max_iter=200, tol=1e-12, fields=True)
    assert not got.status.any() and not got.tangent_info.any()
    eq = law.host_history(got.strain, got.flux, d["coef"], d["rows"][:, :3], d["points"], history=np.zeros_like(h))[:, :, 0]  # max(0, eq)
    assert (np.abs(eq - h[:, :, 0]) > 1e-3).all() and (eq > h[:, :, 0]).any() and (eq < h[:, :, 0]).any()
    step, worst = 1e-5, 0.0
    for c in range(NC):
        F = np.zeros((p.t, p.t))
        for j in range(p.t):
            e = np.zeros(p.t)
            e[j] = step
            flux = [HR.iterate(solve, law, d["coef"][c], d["xi"][c] + s * e, h[c], d["M"][c], d["rows"][c, :3], d["points"], max_iter=200,
                               tol=1e-14)["mean_flux"] for s in (1.0, -1.0)]
            F[:, j] = (flux[0] - flux[1]) / (2 * step)
        worst = max(worst, np.abs(got.tangent[c] - F).max() / np.abs(F).max())
    apart = np.abs(got.tangent - got.A_eff).max() / np.abs(got.tangent).max()
    print(f"{shape}: |D - FD| = {worst:.3e} of the largest entry; D against the secant tensor {apart:.3f}; asymmetry {got.asymmetry.max():.1e}")
    assert worst <= 1e-8
    assert apart > 0.01 and np.all(got.asymmetry <= 1e-14)


@pytest.mark.parametrize("shape", ["p2", "e2", "mesh_p2"])
def test_under_unloading_the_tangent_is_the_secant_tensor(shape):
    p, d = _case(shape, 1)
    law = damage_law(p.kind, p.dim)
    loaded = _run(p, d, law, 0.0, max_iter=100, tol=1e-12)
    assert not loaded.status.any()
    dd = dict(d, xi=0.5 * d["xi"])
    r = _tangent(p, dd, law, shape, loaded.history, max_iter=100, tol=1e-12)
    assert not r.status.any() and np.array_equal(r.rounds, np.full(NC, 2)) and np.array_equal(r.history, loaded.history)
    dev = np.abs(r.tangent - r.A_eff).max() / np.abs(r.A_eff).max()
    print(f"{shape}: unloading, |tangent - A_eff| = {dev:.3e} of the largest entry; asymmetry {r.asymmetry.tolist()}")
    assert dev <= 1e-12 and np.all(r.asymmetry == 0.0)


# -- g. the slot path: a field that does not fit LDS beside the stack ----------------------------------------------------------------------
def test_slot_path_and_lds_path_on_a_large_cell():
    from hommx_amd import MicroCellPlan

    n = 112  # 8 ndof = 98 KiB: with the 60 KiB of fifteen stack rows above the 150 KiB limit of the reconstruction, with four below it
    p = MicroCellPlan(2, n, "poisson")
    rng = np.random.default_rng(12)
    d = {"coef": np.exp(rng.uniform(-1, 1, (1, p.n_el))), "xi": rng.standard_normal((1, 2)), "M": None,
         "rows": rng.integers(-8, 9, (1, 4)) / 8.0, "points": rng.integers(0, 17, (p.n_el, 2)) / 16.0}
    h = rng.integers(0, 16, (1, p.n_el, 1)) / 8.0
    text = "max(h[0], e[0]**2)"
    for _ in range(12):
        text = f"(1 + {text})"
    update = ["max(h[0], abs(e[0]))"]
    deep, shallow = _law([f"c[0]/{text}"], history=update), _law(["c[0]/(1 + max(h[0], e[0]**2))"], history=update)
    assert deep.depth == 16 and shallow.depth <= 5 and 8 * n * n + 4096 * 15 > 150 * 1024 >= 8 * n * n + 4096 * 4
    for name, law in (("slot", deep), ("lds", shallow)):
        r = _run(p, d, law, h, max_iter=2, tol=0.0, fields=True, values=True, return_coef=True)
        assert not r.info.any() and r.rounds[0] == 2 and r.status[0] == 1
        args = (r.strain, r.flux, d["coef"], d["rows"][:, :3])
        assert np.array_equal(r.values, law.host_values(*args, history=h)), name
        assert np.array_equal(r.history, law.host_history(*args, history=h)), name
        assert (r.history > h).any() and (r.history == h).any()
        A = p.solve(r.coef)
        assert np.abs(A - r.A_eff).max() <= 1e-12 * np.abs(A).max(), name
    p.close()


# -- h. the solver classes -----------------------------------------------------------------------------------------------------------------
def test_poisson_hmm_loads_unloads_and_reloads_with_both_methods():
    from hommx_amd import fem, hmm, mesh

    law = hmm.SecantLaw(f"c[0]*{G}", history=[KAPPA], history_names=("kappa",))

    def path(method):
        A = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1]) + 0.1 * x[0]
        h = hmm.PoissonHMM(mesh.create_unit_square(4, 4), A, lambda x: 0.0 * x[0], mesh.create_unit_square(5, 5), 0.05)
        V = h.function_space
        nodes = hmm._box_boundary_nodes(V.mesh)
        us, steps, u = [], [], None
        for scale in (1.0, 0.5, 1.5):  # load, unload, reload: the boundary values alone drive the macro gradient
            g = fem.Function(V)
            g.x.array[:] = scale * (V.mesh.geometry.x[:, 0] + 0.5 * V.mesh.geometry.x[:, 1] ** 2)
            h.set_boundary_conditions(fem.dirichletbc(g, nodes, V))
            u = h.solve_nonlinear(law, max_iter=60, tol=1e-11, micro_iter=100, micro_tol=1e-13, method=method, u0=u).x.array.copy()
            assert not h.secant.status.any() and h.nonlinear_history[-1] <= 1e-11
            if scale == 0.5:
                assert np.array_equal(h.history_trial, h.history)  # unloading: not a bit
            else:
                assert (h.history_trial >= (0.0 if h.history is None else h.history)).all()
            h.commit_history()
            us.append(u)
            steps.append(len(h.nonlinear_history))
        assert h.history.shape == (32, 50, 1) and np.array_equal(h.history_cells, np.arange(32))
        return us, steps, h.history.copy()

    (us, ss, hs), (un, sn, hn) = path("secant"), path("newton")
    print(f"macro steps: secant {ss}, newton {sn}")
    for k in range(3):
        dev = np.abs(us[k] - un[k]).max() / np.abs(us[k]).max()
        print(f"load step {k}: newton against secant {dev:.3e}")
        assert dev <= 1e-8
    assert np.abs(hs - hn).max() <= 1e-8 * np.abs(hs).max()
    assert sn[0] < ss[0]  # Newton takes fewer macro steps on the loading step
