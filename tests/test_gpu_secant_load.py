"""A load beside a strain-dependent law on the device (-m gpu; k_secant_load of csrc/secant_load.hip, k_secant_tangent_load of
csrc/secant_tangent_load.hip, hommx_secant_load_source, hommx_secant_tangent_load_source), on the six shapes of
test_gpu_elem_walk_bits.py, three seeded cells each, with and without M: every (DIM, KIND, MESH) class of the two kernels and the three
routes of the load solve (fused substitution on ``p2``, the blocked pass, the frontal mesh plans with ``load_solve=True``).  Held:

a. a zero polarisation and a zero eigenstrain give the unloaded call's outputs as numbers;
b. the law bit for bit: ``host_values`` fed with the strain, the flux and the base coefficient of the same call reproduces ``values``
   for a program of exactly rounded operations -- the strain and flux the law READ, total or elastic;
c. four rounds against tests/secant_load_ref.py: the coefficient and A_eff to 1e-9 of the largest entry, the bound of test_gpu_secant.py
   for the same comparison; at tol = 1e-10 every cell stops in the reference's round;
d. on ``coef_out``: mean_flux - A_eff xi is Levin's effective polarisation of ``loads_ref.Cell``; strain and flux are those of
   ``criterion(coef_out, P=..., fields=True)`` (an eigenstrain: strain + E is the criterion's total strain), 1e-9 of the largest entry;
e. the two laminates of the section against their scalar layer equations to 1e-9;
f. chunking, batch position, ``max_iter`` beyond the stopping round, the outputs asked for and the entry change no bit;
g. ``secant_tangent`` with a load against the reference tangent to 1e-9 and against central differences of the device's own
   ``mean_flux`` (h = 1e-5, 1e-8 of max |D|: the step and bound of the unloaded reference, test_secant_tangent_host.py);
h. one history case against the reference; unloading changes no bit of the history;
i. the solver classes end to end.

No stream is created here (DESIGN 4.15 records why): the device entry runs on the current stream.
"""

import functools

import numpy as np
import pytest

import secant_load_ref as SL
import secant_tangent_ref as TR
from test_gpu_elem_walk_bits import NC, SHAPES
from test_gpu_secant import CASES, _bits, _case, _plan, _same, exact_law, soft_law
from test_gpu_secant_history import damage_law
from test_gpu_secant_tangent import _mesh, _sibling
from test_secant_load_host import layer_value

pytestmark = pytest.mark.gpu

CODES = [False, True]  # eigenstrain
IDS = ["P", "E"]


@functools.lru_cache(maxsize=None)
def _load(shape, with_M):
    """One seeded load per cell, of order 0.3 with a non-zero mean: it moves every strain by an amount of the order of the strain."""
    p = _plan(shape)
    rng = np.random.default_rng(9900 + 10 * list(SHAPES).index(shape) + with_M)
    a = 0.3 * rng.standard_normal((NC, p.n_el, p.t)) + 0.2 * rng.standard_normal((NC, 1, p.t))
    a.setflags(write=False)
    return a


def _run(p, d, law, load, eigenstrain, **kw):
    rows = d["rows"][:, :3 + law.n_fields]
    return p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, points=d["points"], P=load, eigenstrain=eigenstrain, **kw)


def _cells(shape):
    dim, kind, n = SHAPES[shape]
    return SL.cells(kind, dim, n) if n else SL.cells(kind, dim, msh=_mesh(dim))


# -- a. a zero load ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape,with_M", CASES)
def test_a_zero_load_gives_the_unloaded_outputs(shape, with_M, eigenstrain):
    p, d = _case(shape, with_M)
    law = soft_law(p.kind, p.dim)
    kw = dict(max_iter=3, tol=0.0, fields=True, values=True, return_coef=True)
    rows = d["rows"][:, :3]
    want = p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, points=d["points"], **kw)
    got = _run(p, d, law, np.zeros((NC, p.n_el, p.t)), eigenstrain, **kw)
    for name in ("A_eff", "mean_flux", "rounds", "change", "status", "info", "coef", "strain", "flux", "values"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name  # as numbers: the sign of a zero may differ


# -- b. the law, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape,with_M", CASES)
def test_exact_program_equals_the_host_twin_bitwise(shape, with_M, eigenstrain):
    p, d = _case(shape, with_M)
    law, load = exact_law(p.kind, p.dim), _load(shape, with_M)
    r = _run(p, d, law, load, eigenstrain, max_iter=1, fields=True, values=True, return_coef=True)
    assert not r.info.any() and np.array_equal(r.rounds, np.ones(NC, dtype=np.int64))
    host = law.host_values(r.strain, r.flux, d["coef"], d["rows"][:, :3], d["points"], d["rows"][:, 3:4])
    assert r.values.shape == host.shape == (NC, p.n_el, p.n_comp)
    assert np.array_equal(r.values, host)
    assert np.array_equal(r.coef, d["coef"])  # a stopping round commits nothing
    plain = p.secant(d["coef"], d["xi"], law, d["M"], rows=d["rows"][:, :4], points=d["points"], max_iter=1, fields=True)
    assert np.array_equal(r.A_eff, plain.A_eff) and not np.array_equal(r.strain, plain.strain)  # the same elimination, another state


# -- c. the iteration against the reference ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(shape, eigenstrain, max_iter, tol):
    """secant_load_ref on the three cells of `shape` with M: computed once, read only."""
    p, d = _case(shape, 1)
    law, make, load = soft_law(p.kind, p.dim), _cells(shape), _load(shape, 1)
    return [SL.iterate(make, law, d["coef"][c], d["xi"][c], load[c], eigenstrain, d["M"][c], max_iter=max_iter, tol=tol) for c in range(NC)]


@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_four_rounds_against_the_reference(shape, eigenstrain):
    p, d = _case(shape, 1)
    r = _run(p, d, soft_law(p.kind, p.dim), _load(shape, 1), eigenstrain, max_iter=4, tol=0.0, return_coef=True)
    ref = _reference(shape, eigenstrain, 4, 0.0)
    assert np.array_equal(r.rounds, np.full(NC, 4)) and np.array_equal(r.status, np.ones(NC, dtype=np.int64)) and not r.info.any()
    for c in range(NC):
        dc = np.abs(r.coef[c] - ref[c]["coef"]).max() / np.abs(ref[c]["coef"]).max()
        dA = np.abs(r.A_eff[c] - ref[c]["A"]).max() / np.abs(ref[c]["A"]).max()
        df = np.abs(r.mean_flux[c] - ref[c]["mean_flux"]).max() / np.abs(ref[c]["mean_flux"]).max()
        print(f"{shape} {IDS[eigenstrain]} cell {c}: fourth iterate, coef {dc:.3e}, A_eff {dA:.3e}, mean_flux {df:.3e} (relative to the largest entry)")
        assert dc <= 1e-9 and dA <= 1e-9


@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_cell_stops_in_the_round_of_the_reference(shape, eigenstrain):
    p, d = _case(shape, 1)
    r = _run(p, d, soft_law(p.kind, p.dim), _load(shape, 1), eigenstrain, max_iter=60, tol=1e-10, return_coef=True)
    ref = _reference(shape, eigenstrain, 60, 1e-10)
    print(f"{shape} {IDS[eigenstrain]}: rounds {r.rounds.tolist()} against {[x['rounds'] for x in ref]} of the reference; change "
          f"{r.change.tolist()} against {[x['change'] for x in ref]}")
    assert all(x["status"] == 0 for x in ref)
    assert not r.status.any() and not r.info.any()
    assert r.rounds.tolist() == [x["rounds"] for x in ref]
    assert np.all(r.change <= 1e-10)


# -- d. the outputs of the stopping round belong together -------------------------------------------------------------------------------
@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_levin_and_the_criterion_on_the_stream_of_the_stopping_round(shape, eigenstrain):
    from hommx_amd.expr import Criterion

    p, d = _case(shape, 1)
    load = _load(shape, 1)
    r = _run(p, d, soft_law(p.kind, p.dim), load, eigenstrain, max_iter=60, tol=1e-10, return_coef=True, fields=True)
    assert not r.status.any()
    make = _cells(shape)
    for c in range(NC):
        cell = make(r.coef[c], d["M"][c])
        P = -np.einsum("emn,en->em", cell.V, load[c]) if eigenstrain else load[c]
        want = cell.levin(P[None])[0]
        got = r.mean_flux[c] - r.A_eff[c] @ d["xi"][c]
        dev = np.abs(got - want).max() / max(np.abs(want).max(), np.abs(r.mean_flux[c]).max())
        print(f"{shape} {IDS[eigenstrain]} cell {c}: |mean_flux - A_eff xi - Levin| = {dev:.3e} of the largest entry")
        assert dev <= 1e-9
    crit = p.criterion(r.coef, d["xi"], Criterion("e[0]"), d["M"], rows=d["rows"][:, :3], points=d["points"], fields=True, P=load,
                       eigenstrain=eigenstrain)
    total = r.strain + load if eigenstrain else r.strain
    for name, got, want in (("strain", total, crit.strain), ("flux", r.flux, crit.flux)):
        dev = np.abs(got - want).max() / np.abs(want).max()
        print(f"{shape} {IDS[eigenstrain]} {name}: deviation from criterion(coef_out) {dev:.3e} of the largest entry")
        assert dev <= 1e-9
    assert np.array_equal(crit.A_eff, r.A_eff)  # the corrector route of the plan on the same stream


# -- e. the laminates -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eigenstrain,rounds", [(True, 9), (False, 8)], ids=["E", "P"])
def test_laminate_against_the_scalar_layer_equations(eigenstrain, rounds):
    from oracle import hommx_oracle as O

    p = _plan("p2")
    x, cells = O.unit_cell_mesh(2, 8)
    stiff = x[cells].mean(axis=1)[:, 0] < 0.25
    base = np.where(stiff, 10.0, 1.0)
    load = np.stack([np.where(stiff, 0.5, -0.2), np.zeros(p.n_el)], axis=-1)
    want = layer_value(eigenstrain)
    r = p.secant(base[None], np.array([[2.0, 0.0]]), soft_law("poisson", 2), max_iter=60, tol=1e-12, P=load[None], eigenstrain=eigenstrain)
    print(f"laminate {IDS[eigenstrain]}: mean_flux[0] = {r.mean_flux[0, 0]!r} after {r.rounds[0]} rounds; layer equations {want!r}")
    assert r.status[0] == 0 and r.rounds[0] == rounds
    assert abs(r.mean_flux[0, 0] - want) <= 1e-9


# -- f. independence, bit for bit -----------------------------------------------------------------------------------------------------------
def _staggered(shape):
    """The batch of `shape` with M, its macro strains and loads scaled by 0.1, 1 and 3: the cells stop in different rounds."""
    p, d = _case(shape, 1)
    s = np.array([0.1, 1.0, 3.0])
    return p, dict(d, xi=d["xi"] * s[:, None]), _load(shape, 1) * s[:, None, None]


@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape", ["p2", "e3", "mesh_p2"])
def test_a_cell_does_not_depend_on_chunking_position_max_iter_or_outputs(shape, eigenstrain, monkeypatch):
    p, d, load = _staggered(shape)
    law = soft_law(p.kind, p.dim)
    want = _run(p, d, law, load, eigenstrain, max_iter=60, return_coef=True)
    print(f"{shape} {IDS[eigenstrain]}: rounds {want.rounds.tolist()}")
    assert not want.status.any() and len(set(want.rounds.tolist())) > 1
    _same(_run(p, d, law, load, eigenstrain, max_iter=60, return_coef=True, fields=True, values=True), want, what="outputs")
    _same(_run(p, d, law, load, eigenstrain, max_iter=60), want, what="no optional output")
    cut = int(want.rounds.min())  # the round the first cell stops in: with status 0, which is tested before status 1
    early = want.rounds <= cut
    assert early.any() and not early.all()
    _same(_run(p, d, law, load, eigenstrain, max_iter=cut, return_coef=True), want, early, "max_iter")
    one = p.secant(d["coef"][1:2], d["xi"][1:2], law, d["M"][1:2], rows=d["rows"][1:2, :3], max_iter=60, return_coef=True, P=load[1:2],
                   eigenstrain=eigenstrain)
    for x, y in zip(_bits(one), _bits(want)):
        assert np.array_equal(x[0], y[1])
    order = [2, 0, 1]
    swapped = p.secant(d["coef"][order], d["xi"][order], law, d["M"][order], rows=d["rows"][order, :3], max_iter=60, return_coef=True,
                       P=load[order], eigenstrain=eigenstrain)
    for x, y in zip(_bits(swapped), _bits(want)):
        assert np.array_equal(x, y[order])
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")
    _plan.cache_clear()  # the variable is read when a plan is created
    try:
        q = _plan(shape)
        rep = 120  # 360 cells: at least two chunks of 1 MB of correctors and load correctors
        tile = lambda a: np.concatenate([a] * rep)
        got = q.secant(tile(d["coef"]), tile(d["xi"]), law, tile(d["M"]), max_iter=60, return_coef=True, P=tile(load), eigenstrain=eigenstrain)
        for x, y in zip(_bits(got), _bits(want)):
            assert np.array_equal(x, tile(y))
        q.close()
    finally:
        _plan.cache_clear()
        _case.cache_clear()
        _load.cache_clear()


@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape", ["p2", "e2", "mesh_ev3"])
def test_device_entry_equals_host_entry(shape, eigenstrain):
    import torch

    from hommx_amd.batch import CoefStream

    p, d, load = _staggered(shape)
    law = soft_law(p.kind, p.dim)
    want = _run(p, d, law, load, eigenstrain, max_iter=60, return_coef=True, fields=True, values=True)
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
    P_ptr = upload(load)
    on_device = keep[-1]
    p.secant_device(NC, CoefStream.sampled(d["coef"]).coef_source(upload), upload(d["M"]), upload(d["xi"]), law, upload(d["rows"][:, :3]),
                    ptr["state"], ptr["A_eff"], max_iter=60, mean_flux_ptr=ptr["mean_flux"], coef_ptr=ptr["coef"], strain_ptr=ptr["strain"],
                    flux_ptr=ptr["flux"], values_ptr=ptr["values"], info_ptr=ptr["info"], stream=torch.cuda.current_stream(dev).cuda_stream,
                    P_ptr=P_ptr, eigenstrain=eigenstrain)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["state"], np.stack([want.rounds, want.change, want.status], axis=1).astype(np.float64))
    for k in ("A_eff", "mean_flux", "coef", "strain", "flux", "values", "info"):
        assert np.array_equal(got[k], getattr(want, k)), k
    assert np.array_equal(on_device.cpu().numpy(), load)  # the load array, an eigenstrain too, is never written


# -- g. the tangent ---------------------------------------------------------------------------------------------------------------------------
def _tangent(p, d, law, shape, load, eigenstrain, **kw):
    rows = d["rows"][:, :3 + law.n_fields]
    return p.secant_tangent(d["coef"], d["xi"], law, _sibling(shape), d["M"], rows=rows, points=d["points"], P=load, eigenstrain=eigenstrain, **kw)


@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape,with_M", CASES)
def test_tangent_against_the_reference(shape, with_M, eigenstrain):
    dim, kind, n = SHAPES[shape]
    p, d = _case(shape, with_M)
    law, dlaw = TR.potential_law(kind, dim)
    load, make = _load(shape, with_M), _cells(shape)
    got = _tangent(p, d, law, shape, load, eigenstrain, max_iter=60, tol=1e-12, return_coef=True)
    plain = _run(p, d, law, load, eigenstrain, max_iter=60, tol=1e-12, return_coef=True)
    _same(got, plain, what="the outputs shared with secant()")
    assert not got.status.any() and not got.tangent_info.any(), (got.status, got.tangent_info)
    worst = 0.0
    for c in range(NC):
        M = None if d["M"] is None else d["M"][c]
        ref = SL.iterate(make, law, d["coef"][c], d["xi"][c], load[c], eigenstrain, M, d["rows"][c, :3], d["points"], max_iter=60, tol=1e-12)
        assert ref["status"] == 0
        D = SL.tangent(kind, dim, dlaw, ref, d["coef"][c], d["xi"][c], M, n=n, msh=None if n else _mesh(dim))["D"]
        worst = max(worst, np.abs(got.tangent[c] - D).max() / np.abs(D).max())
    print(f"{shape} M={with_M} {IDS[eigenstrain]}: rounds {got.rounds}, |D - D_ref| = {worst:.3e} of the largest entry, asymmetry "
          f"{got.asymmetry.max():.1e}")
    assert worst <= 1e-9
    assert np.all(got.asymmetry <= 1e-14)


@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
@pytest.mark.parametrize("shape", ["p2", "e2", "mesh_p2"])
def test_tangent_against_central_differences_of_the_devices_mean_flux(shape, eigenstrain):
    dim, kind, _ = SHAPES[shape]
    p, d = _case(shape, 1)
    law, _ = TR.potential_law(kind, dim)
    load, h = _load(shape, 1), 1e-5
    kw = dict(max_iter=200, tol=1e-14)
    got = _tangent(p, d, law, shape, load, eigenstrain, **kw)
    assert set(np.unique(got.status)) <= {0, 1}  # at tol = 1e-14 a cell may sit on its rounding floor until max_iter: the state is the same
    F = np.zeros((NC, p.t, p.t))
    for j in range(p.t):
        step = np.zeros(p.t)
        step[j] = h
        fp = _run(p, dict(d, xi=d["xi"] + step), law, load, eigenstrain, **kw).mean_flux
        fm = _run(p, dict(d, xi=d["xi"] - step), law, load, eigenstrain, **kw).mean_flux
        F[:, :, j] = (fp - fm) / (2 * h)
    err = np.abs(got.tangent - F).max(axis=(1, 2)) / np.abs(got.tangent).max(axis=(1, 2))
    apart = np.abs(got.tangent - got.A_eff).max() / np.abs(got.tangent).max()
    print(f"{shape} {IDS[eigenstrain]}: |D - FD| = {err.max():.2e} of max |D|; D against the secant tensor: {apart:.2f}")
    assert np.all(err <= 1e-8)
    assert apart > 0.01


# -- h. history variables -------------------------------------------------------------------------------------------------------------------
def test_damage_with_an_eigenstrain_against_the_reference_and_unloading_keeps_the_history():
    shape = "p2"
    p, d = _case(shape, 1)
    law, make, E = damage_law(p.kind, p.dim), _cells(shape), _load(shape, 1)
    h0 = np.zeros((NC, p.n_el, 1))
    kw = dict(max_iter=100, tol=1e-10, return_coef=True)
    r = _run(p, d, law, E, True, history=h0, **kw)
    assert not r.status.any() and not r.info.any() and (r.history > 0).all()
    for c in range(NC):
        ref = SL.iterate(make, law, d["coef"][c], d["xi"][c], E[c], True, d["M"][c], d["rows"][c, :3], d["points"], max_iter=100, tol=1e-10,
                         history=h0[c])
        dA = np.abs(r.A_eff[c] - ref["A"]).max() / np.abs(ref["A"]).max()
        dh = np.abs(r.history[c] - ref["history"]).max() / np.abs(ref["history"]).max()
        print(f"cell {c}: rounds {r.rounds[c]} against {ref['rounds']}; A_eff {dA:.3e}, history {dh:.3e} (relative to the largest entry)")
        assert ref["status"] == 0 and abs(int(r.rounds[c]) - ref["rounds"]) <= 1
        assert dA <= 1e-9 and dh <= 1e-9
    half = _run(p, dict(d, xi=0.5 * d["xi"]), law, 0.5 * E, True, history=r.history, **kw)  # the macro strain and the eigenstrain recede
    print(f"unloading: rounds {half.rounds.tolist()}")
    assert not half.status.any()
    assert np.array_equal(half.history, r.history)  # not a bit
    again = _tangent(p, d, law, shape, E, True, history=h0, **kw)
    assert np.array_equal(again.history, r.history) and np.array_equal(again.A_eff, r.A_eff)


# -- i. the solver classes ------------------------------------------------------------------------------------------------------------------
def _poisson_solver():
    from hommx_amd import hmm, mesh

    A = hmm.TwoPhase(lambda y: (y[0] - 0.5) ** 2 + (y[1] - 0.5) ** 2 < 0.09, lambda x: 10.0 + 0.0 * x[0], lambda x: 1.0 + 0.0 * x[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(6, 6), A, lambda x: 20.0 + 0.0 * x[0], mesh.create_unit_square(8, 8), 0.05)
    h.set_eigenstrain(lambda x, y: [0.3 + 0.2 * x[0] + 0.1 * np.sin(2 * np.pi * y[1]), -0.2 + 0.0 * x[0] * y[0]])
    return h


def test_poisson_hmm_with_an_eigenstrain_both_methods_and_the_identity_law():
    from hommx_amd import hmm

    h = _poisson_solver()
    u = h.solve().x.array.copy()
    v = h.solve_nonlinear(hmm.SecantLaw("c[0]"), load=True).x.array
    assert len(h.nonlinear_history) == 1 and h.nonlinear_history[0] <= 1e-12
    assert np.abs(u - v).max() <= 1e-12 * np.abs(u).max()
    law, tol = hmm.SecantLaw("c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"), 1e-10
    us = h.solve_nonlinear(law, max_iter=80, tol=tol, micro_tol=1e-13, micro_iter=200, load=True).x.array.copy()
    hs, Ps = list(h.nonlinear_history), h.effective_polarisation.copy()
    un = h.solve_nonlinear(law, max_iter=80, tol=tol, micro_tol=1e-13, micro_iter=200, load=True, method="newton").x.array.copy()
    dev = np.abs(un - us).max() / np.abs(us).max()
    print(f"secant {len(hs)} steps, newton {len(h.nonlinear_history)} steps, |u_newton - u_secant| = {dev:.2e} of max |u|")
    assert hs[-1] <= tol and h.nonlinear_history[-1] <= tol and len(hs) > 2 and not h.secant.status.any()
    assert dev <= 100 * tol  # each loop stops within tol / (1 - its contraction rate) of the solution; the secant loop's rate is below 0.99
    assert np.abs(h.effective_polarisation - Ps).max() <= 100 * tol * np.abs(Ps).max()
    assert np.abs(us - u).max() > 1e-3 * np.abs(u).max()  # the law matters


def test_elasticity_hmm_with_a_thermal_expression_solves_its_own_secant_system():
    from hommx_amd import fem, hmm, mesh

    A = hmm.TwoPhase(lambda y: y[0] < 0.5, lambda x: hmm.Lame(20.0 + 0.0 * x[0], 10.0 + 0.0 * x[0]),
                     lambda x: hmm.Lame(2.0 + 0.0 * x[0], 1.0 + 0.0 * x[0]))
    h = hmm.LinearElasticityHMM(mesh.create_unit_square(4, 4), A, lambda x: np.array([0.0, -8.0]), mesh.create_unit_square(5, 5), 0.05)
    V = h.function_space
    clamp = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1) | np.isclose(x[1], 0) | np.isclose(x[1], 1))
    h.set_boundary_conditions(fem.dirichletbc(fem.Function(V), clamp, V))
    alpha = hmm.Expression(["where(y[0] < 0.5, 0.01, 0.03)*f[0]", "where(y[0] < 0.5, 0.01, 0.03)*f[0]", "0*f[0]"], fields=("dT",))
    h.set_eigenstrain(alpha)
    h.set_polarisation_fields(10.0 + 20.0 * h._msh.cell_midpoints()[:, 0])
    assert h._loads_on_device(h._coef_stream(np.arange(1))[1])  # the program path: HOMMX_LOADS_PROGRAM | HOMMX_LOADS_EIGENSTRAIN
    tol = 1e-8
    law = hmm.SecantLaw(lam="c[0]", mu="c[1]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))")
    u = h.solve_nonlinear(law, max_iter=60, tol=tol, load=True).x.array.copy()
    assert h.nonlinear_history[-1] <= tol and len(h.nonlinear_history) > 2 and not h.secant.status.any()
    cells = np.arange(h._msh.num_cells)
    h._set_macro_matrix(h._local_stiffness_from_tensors(cells, h.effective_tensors))
    h._linearisation_load, h._nonlinear_load = h.effective_polarisation, True
    try:
        v = h.solve().x.array.copy()
    finally:
        h._linearisation_load, h._nonlinear_load = None, False
        h._needs_reassembly = True
    dev = np.abs(u - v).max() / np.abs(v).max()
    print(f"thermal elasticity: {len(h.nonlinear_history)} macro steps, |u - solve(secant tensors, effective polarisations)| = {dev:.3e}")
    assert dev <= 10 * tol
    assert np.abs(h.effective_polarisation).max() > 0.01  # the thermal strain loads the macro problem


# -- j. the slot path: the field behind TWO corrector blocks, and under the tangent kernel ------------------------------------------------
LOADS = [None, False, True]  # no load, a polarisation, an eigenstrain
LOAD_IDS = ["none", "P", "E"]


@functools.lru_cache(maxsize=None)
def _large_cell():
    """The cell of test_slot_path_and_lds_path_on_a_large_cell (test_gpu_secant.py) with its two laws and one seeded load: n = 112, so
    that the field of 8 n n bytes = 98 KiB fits the 150 KiB of LDS beside the stack rows of the shallow law and not beside those of
    the depth-16 law -- fifteen rows of 4096 bytes (512 threads) under the round kernel, fifteen of (1 + P) times that under the
    tangent kernel."""
    from hommx_amd import MicroCellPlan

    from test_gpu_secant import _law

    n = 112
    p = MicroCellPlan(2, n, "poisson")
    rng = np.random.default_rng(12)
    d = {"coef": np.exp(rng.uniform(-1, 1, (1, p.n_el))), "xi": rng.standard_normal((1, 2)), "M": None,
         "rows": rng.integers(-8, 9, (1, 4)) / 8.0, "points": rng.integers(0, 17, (p.n_el, 2)) / 16.0}
    d["load"] = 0.3 * rng.standard_normal((1, p.n_el, p.t)) + 0.2 * rng.standard_normal((1, 1, p.t))
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    text = "e[0]**2"
    for _ in range(13):
        text = f"(1 + {text})"
    deep, shallow = _law([f"c[0]/{text}"]), _law(["c[0]/(1 + e[0]**2)"])
    assert deep.depth == 16 and shallow.depth <= 4
    return p, d, (("slot", deep), ("lds", shallow))


@pytest.mark.parametrize("eigenstrain", CODES, ids=IDS)
def test_slot_path_and_lds_path_beside_a_load_on_a_large_cell(eigenstrain):
    """The rounds of k_secant_load with the field in global scratch: the slot lies behind the canonical corrector blocks AND the block
    of the load's corrector.  The assertions are those of the unloaded test, on the strain and flux the law read."""
    p, d, laws = _large_cell()
    n = p.n_micro
    assert 8 * n * n + 4096 * 15 > 150 * 1024 >= 8 * n * n + 4096 * 3  # the branch of the round kernel, as in the unloaded test
    for name, law in laws:
        r = _run(p, d, law, d["load"], eigenstrain, max_iter=2, tol=0.0, fields=True, values=True, return_coef=True)
        assert not r.info.any() and r.rounds[0] == 2 and r.status[0] == 1
        first = _run(p, d, law, d["load"], eigenstrain, max_iter=1, fields=True, values=True)
        assert np.array_equal(first.values, law.host_values(first.strain, first.flux, d["coef"], d["rows"][:, :3])), name
        assert np.array_equal(r.coef, first.values[..., 0]), name
        assert np.array_equal(r.values, law.host_values(r.strain, r.flux, d["coef"], d["rows"][:, :3])), name
        A = p.solve(r.coef)
        assert np.abs(A - r.A_eff).max() <= 1e-12 * np.abs(A).max(), name


@pytest.mark.parametrize("eigenstrain", LOADS, ids=LOAD_IDS)
def test_tangent_tail_on_the_slot_path_and_the_lds_path_of_a_large_cell(eigenstrain):
    """k_secant_tangent / k_secant_tangent_load with the field in global scratch, behind one corrector block set or two.  Which branch a
    law takes follows from secant_tangent_lds_bytes = 8 (ndof + 512 (1 + P) (depth - 1)) against the 150 KiB limit, P from
    secant_tangent_slots: t = 2 strain entries per sweep where the stack rows of that width fit the limit on their own, else 1."""
    from hommx_amd import MicroCellPlan

    p, d, laws = _large_cell()
    n, row, limit = p.n_micro, 4096, 150 * 1024
    assert 3 * row * 15 > limit >= 2 * row * 15  # depth 16: rows three doubles wide do not fit even without a field, so P = 1 ...
    assert 8 * n * n + 2 * row * 15 > limit  # ... and beside those rows the field does not fit: the slot
    assert 8 * n * n + 3 * row * 3 <= limit  # depth <= 4: P = 2 and the field in LDS
    sib = MicroCellPlan(2, n, p.tangent_kind)
    # the flux c e0 / (1 + e0^2) of the shallow law has a positive tangent for |e0| < 1 only, and the sibling plan eliminates a
    # definite stream: a quarter of the seeded macro strain and load keeps every element there (tangent_info == 0 below says so)
    xi, load = 0.25 * d["xi"], None if eigenstrain is None else 0.25 * d["load"]
    for name, law in laws:
        got = p.secant_tangent(d["coef"], xi, law, sib, None, rows=d["rows"][:, :3], points=d["points"], P=load,
                               eigenstrain=bool(eigenstrain), max_iter=2, tol=0.0, fields=True, return_coef=True, return_tangent_coef=True)
        assert not got.info.any() and got.rounds[0] == 2 and got.status[0] == 1, name
        T, asym = law.host_tangent(got.strain, got.coef, d["coef"], d["rows"][:, :3], d["points"])
        want = np.stack([TR.tangent_stream("poisson", 2, T[c]) for c in range(len(T))])
        assert np.array_equal(got.tangent_coef, want) and np.array_equal(got.asymmetry, asym), name
        D, info = sib.solve(got.tangent_coef, return_info=True)
        assert np.array_equal(info, got.tangent_info) and not info.any(), name
        dev = np.abs(D - got.tangent).max() / np.abs(D).max()
        print(f"{name} {LOAD_IDS[LOADS.index(eigenstrain)]}: tangent against solve(tangent_coef): {dev:.3e}")
        assert dev <= 1e-12, name
    sib.close()
