"""Accuracy of the nonlinear family against extended precision, on an MI355X (-m gpu; DESIGN 4.11 "Nonlinear outputs"): the secant
iteration at a fixed round and at its fixed point, the consistent tangent, history variables over three load steps, a load beside the law
on the three load routes, criteria and region rows of the stopped state, the magnitude of the coefficient and the slot path.

For every returned array of every cell   e = max|gpu - T| / max|T|  <=  32 * max(e_float64, 16 eps),   T the long-double truth of
tests/nonlinear_truth.py, e_float64 the error of the float64 references of the coarse tests (secant_ref, history_ref, secant_load_ref,
secant_tangent_ref, secant_state_ref) against the same truth on the same inputs, the same number of rounds.  No bound here is computed
from a device result; tests/test_nonlinear_truth_host.py keeps every yardstick below 1e-11 (strain and flux fields and the history: 1e-10) and the comparisons well-posed.
Everything goes through the Python layer and hence the C ABI.  ``tol = 0`` everywhere, ``max_iter`` the truth's own round count: a
float64 change of exactly zero stops a cell early, so status 0 and 1 are both accepted, and ``rounds`` and ``change`` are never compared.
Every test prints its worst ratio e / (bound / 32); 32 is the limit.
"""

import functools
import time

import numpy as np
import pytest

import accuracy_gpu as G
import accuracy_ref as R
import nonlinear_truth as NT

pytestmark = pytest.mark.gpu

LD = R.LD

ITERATION = ("coef", "A", "mean_flux", "strain", "flux", "values")
TANGENT = ITERATION + ("D", "tangent_coef")
_T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntest_gpu_accuracy_nonlinear.py: {time.perf_counter() - _T0:.1f} s wall time")


@functools.lru_cache(maxsize=None)
def _plan(shape, n=None):
    return G.nonlinear_plan(shape, n)


@functools.lru_cache(maxsize=None)
def _sibling(shape):
    return G.nonlinear_sibling(shape, _plan(shape))


def _one(a, c):
    return None if a is None else a[c:c + 1]


class Held:
    """Collects the comparisons of one test: every quantity of every cell against its own bound.  ``LOG``: one record per finished test
    with every comparison's figures (tools/accuracy_table.py --nonlinear writes them to profiles/accuracy_nonlinear.json)."""

    LOG = []

    def __init__(self):
        self.worst, self.where, self.failures, self.count, self.rows = 0.0, "", [], 0, []

    def arrays(self, what, got: dict, truth: dict, y: dict, names):
        assert got["info"] == 0 and got["status"] in (0, 1), (what, got["status"], got["info"])
        for name in names:
            self.one(what, name, got[name].reshape(np.shape(truth[name])), truth[name], y)

    def one(self, what, name, got, truth, y, key=None):
        err, bound = R.rel(got, truth), y["bound"][key or name]
        ratio = err / (bound / R.FACTOR)
        self.count += 1
        self.rows.append({"at": what, "quantity": name, "e": err, "e_float64": float(y["e"][key or name]), "bound": float(bound), "ratio": ratio})
        if ratio > self.worst:
            self.worst, self.where = ratio, f"{what} {name}"
        if not err <= bound:
            self.failures.append((what, name, f"e {err:.2e}", f"float64 {y['e'][key or name]:.1e}", f"bound {bound:.1e}", f"ratio {ratio:.1f}"))

    def done(self, title):
        print(f"{title}: {self.count} comparisons, worst ratio {self.worst:.2f} ({self.where})")
        Held.LOG.append({"test": title, "worst_ratio": self.worst, "worst_at": self.where, "comparisons": self.rows})
        assert not self.failures, self.failures
        assert self.count


def _secant(shape, c, law, inputs, rounds, **kw):
    coef, M, xi = inputs
    return G.secant_outputs(_plan(shape).secant(_one(coef, c), _one(xi, c), law, _one(M, c), max_iter=rounds, tol=0.0, fields=True,
                                                values=True, return_coef=True, **kw))


def _tangent(shape, c, law, inputs, rounds, **kw):
    coef, M, xi = inputs
    r = G.secant_outputs(_plan(shape).secant_tangent(_one(coef, c), _one(xi, c), law, _sibling(shape), _one(M, c), max_iter=rounds, tol=0.0,
                                                     fields=True, values=True, return_coef=True, return_tangent_coef=True, **kw))
    assert r["tangent_info"] == 0
    return r


# -- the iteration ---------------------------------------------------------------------------------------------------------------------------
_ITER_IDS = [f"{s}-{NT.FAMILY_IDS[fi]}" for s, fi in NT.ITERATION_CASES]


@pytest.mark.parametrize("shape,fi", NT.ITERATION_CASES, ids=_ITER_IDS)
def test_fourth_round(shape, fi):
    """secant(max_iter=4, tol=0) with relax = 1 and relax = 0.5 against the fourth round of the truth: both cells in one call."""
    p = _plan(shape)
    coef, M, xi = NT.inputs(shape, fi)
    law = G.secant_law(NT.soft_law(p.kind, p.dim))
    held = Held()
    for relax in NT.RELAX:
        r = p.secant(coef, xi, law, M, max_iter=4, tol=0.0, relax=relax, fields=True, values=True, return_coef=True)
        assert not r.info.any() and set(r.status.tolist()) <= {0, 1}
        for c in range(NT.NC):
            T, y = NT.iteration_reference(shape, fi, c, relax, 4)
            got = {k: np.asarray(getattr(r, a)[c]) for k, a in G.SECANT_OUTPUTS.items() if getattr(r, a) is not None}
            held.arrays(f"cell {c} relax {relax}", got, T, y, ITERATION)
    held.done(f"{shape} {NT.FAMILY_IDS[fi]} fourth round")


@pytest.mark.parametrize("shape,fi", NT.ITERATION_CASES, ids=_ITER_IDS)
def test_fixed_point(shape, fi):
    """secant(max_iter=R, tol=0), R the truth's own round count (its remainder is then below eps_ld), against the truth's fixed point."""
    p = _plan(shape)
    law = G.secant_law(NT.soft_law(p.kind, p.dim))
    held = Held()
    for c in range(NT.cells_of(shape)):
        T, y = NT.iteration_reference(shape, fi, c)
        held.arrays(f"cell {c} ({T['rounds']} rounds)", _secant(shape, c, law, NT.inputs(shape, fi), T["rounds"]), T, y, ITERATION)
    held.done(f"{shape} {NT.FAMILY_IDS[fi]} fixed point")


def test_laminate_against_mpmath():
    """b = 10 on y0 < 0.25, xi = (2, 0): A_H[0][0] against the root of the two layer equations in mpmath, at the bound of the
    float64 reference's own error against it (nonlinear_truth.laminate_reference; capped by the host test)."""
    base, xi, _ = NT.laminate()
    T, want, y = NT.laminate_reference()
    r = _plan("p2").secant(base[None], xi[None], G.secant_law(NT.soft_law("poisson", 2)), max_iter=T["rounds"], tol=0.0)
    assert r.status[0] in (0, 1) and not r.info.any()
    print(f"laminate: A_H[0][0] = {r.A_eff[0, 0, 0]!r}, mpmath {want!r}")
    held = Held()
    held.one(f"{T['rounds']} rounds", "A00", r.A_eff[0, 0, 0], want, y)
    held.done("laminate")


# -- the tangent -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fi", NT.TANGENT_CASES, ids=[f"{s}-{NT.FAMILY_IDS[fi]}" for s, fi in NT.TANGENT_CASES])
def test_tangent(shape, fi):
    """secant_tangent at the fixed point of a potential law: the iteration's outputs, ``tangent`` (D) and ``tangent_coef``; the element
    tangents are symmetric (asymmetry <= 1e-14, the demand of test_gpu_secant_tangent.py) and so is D, to its bound."""
    p = _plan(shape)
    law = G.secant_law(NT.potential_law(p.kind, p.dim))
    held = Held()
    for c in range(NT.cells_of(shape)):
        T, D, y = NT.tangent_reference(shape, fi, c)
        r = _tangent(shape, c, law, NT.inputs(shape, fi, NT.tangent_xi(shape)), T["rounds"])
        held.arrays(f"cell {c}", r, dict(T, **D), y, TANGENT)
        assert r["asymmetry"] <= 1e-14
        assert np.abs(r["D"] - r["D"].T).max() <= y["bound"]["D"] * np.abs(r["D"]).max()
    held.done(f"{shape} {NT.FAMILY_IDS[fi]} tangent")


def test_asymmetry_of_a_law_without_a_potential():
    shape, fi = NT.ASYMMETRIC_CASE
    p = _plan(shape)
    law = G.secant_law(NT.potential_law(p.kind, p.dim, True))
    held = Held()
    for c in range(NT.NC):
        T, D, y = NT.tangent_reference(shape, fi, c, True)
        r = _tangent(shape, c, law, NT.inputs(shape, fi, NT.tangent_xi(shape)), T["rounds"])
        held.arrays(f"cell {c}", r, dict(T, **D), y, TANGENT + ("asymmetry",))
    held.done(f"{shape} asymmetric law")


# -- history -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NT.HISTORY_SHAPES)
def test_history_over_three_load_steps(shape):
    """Load, increase, unload as three chained calls: the device's history of one step feeds the next, the truth chains its own.
    history, A_eff, mean_flux, coef and the tangent of every step; unloading: the history keeps its bits and D meets A_eff."""
    p = _plan(shape)
    law = G.secant_law(NT.damage_law(p.kind, p.dim))
    coef, M, xi = NT.inputs(shape, NT.HISTORY_FAMILY)
    held = Held()
    for c in range(NT.NC):
        h = np.zeros((1, p.n_el, 1))
        for k, ((T, D, y), scale) in enumerate(zip(NT.history_reference(shape, c), NT.HISTORY_STEPS)):
            r = _tangent(shape, c, law, (coef, M, scale * xi), T["rounds"], history=h)
            names = TANGENT + ("history",) + (("asymmetry",) if "asymmetry" in y["e"] else ())
            held.arrays(f"cell {c} step {k}", r, dict(T, **D), y, names)
            if k == 2:
                assert np.array_equal(r["history"], h[0])  # not a bit
                held.one(f"cell {c} unloading", "tangent against A_eff", r["D"], r["A"], y, "D")
            h = r["history"][None]
    held.done(f"{shape} history")


@pytest.mark.parametrize("shape", NT.HISTORY_TANGENT_SHAPES)
def test_tangent_at_frozen_history(shape):
    p = _plan(shape)
    law = G.secant_law(NT.potential_damage_law(p.kind, p.dim))
    held = Held()
    for c in range(NT.NC):
        T, D, y = NT.frozen_reference(shape, c)
        r = _tangent(shape, c, law, NT.inputs(shape, NT.HISTORY_FAMILY), T["rounds"], history=NT.history_start(shape)[c:c + 1])
        held.arrays(f"cell {c}", r, dict(T, **D), y, TANGENT + ("history",))
        assert r["asymmetry"] <= 1e-14
    held.done(f"{shape} frozen history")


# -- loads -------------------------------------------------------------------------------------------------------------------------------------
def _hold_loads(results, shapes, title):
    held = Held()
    for shape in shapes:
        for c in range(NT.cells_of(shape)):
            for eig in (False, True):
                T, D, y = NT.load_reference(shape, c, eig)
                got = {k.split("|")[4]: v for k, v in results.items() if k.startswith(f"nl|{shape}|{c}|{int(eig)}|")}
                assert got["tangent_info"] == 0 and got["asymmetry"] <= 1e-14
                held.arrays(f"{shape} cell {c} {'E' if eig else 'P'}", got, dict(T, **D), y, TANGENT)
    held.done(title)


@pytest.fixture(scope="module")
def loads():
    return G.run_nonlinear_group()


@pytest.mark.parametrize("shape", NT.LOAD_SHAPES)
def test_loads_beside_a_law(loads, shape):
    """A polarisation and an eigenstrain on the three load routes -- fused substitution (p2), the blocked pass (e3), the frontal mesh
    plan with its load solve (mesh_ev3): the iteration's outputs at the fixed point (strain and flux as the law read them) and D."""
    _hold_loads(loads, [shape], f"{shape} loads")


def test_loads_of_the_fused_plan_on_the_blocked_route(tmp_path_factory):
    """HOMMX_FUSED_LOADS=0 (read when a plan is created: one child process, route asserted by the runner): the two p2 cases once more."""
    got = G.run_in_child("nonlinear", "blocked_loads", tmp_path_factory.mktemp("nonlinear_blocked_loads"))
    _hold_loads(got, ["p2"], "p2 loads on the blocked route")


# -- the state tail --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(NT.STATE_CASES))
def test_state_tail(shape):
    """secant(criterion=, reconstruct=, regions=) on p2 with history and eigenstrain, e2 with a polarisation, pm3 with neither (the
    reconstruction takes no load): the criterion's values, max, mean and exceed_volume, the total fields, the region rows; the element
    named as the maximum is the truth's (the host test holds its lead at 1e-9 or more)."""
    p = _plan(shape)
    coef, M, xi = NT.inputs(shape, 0)
    law, crit, hist, load, eig, labels = NT.state_case(shape)
    law64, crit64 = G.secant_law(law), G.criterion(crit)
    held = Held()
    for c in range(NT.NC):
        T, S, y = NT.state_reference(shape, c)
        kw = {}
        if hist is not None:
            kw["history"] = hist[c:c + 1]
        if load is not None:
            kw.update(P=load[c:c + 1], eigenstrain=eig)
        if labels is not None:
            kw.update(reconstruct=True, regions=labels, n_regions=2)
        r = p.secant(_one(coef, c), _one(xi, c), law64, _one(M, c), max_iter=T["rounds"], tol=0.0, fields=True, values=True,
                     return_coef=True, criterion=crit64, crit_values=True, crit_fields=True, **kw)
        got = G.secant_outputs(r)
        held.arrays(f"cell {c}", got, T, y, ITERATION + (("history",) if hist is not None else ()))
        k = r.criterion
        for name, v in (("crit_values", k.values[0]), ("max", k.max[0]), ("mean", k.mean[0]), ("exceed_volume", k.exceed_volume[0]),
                        ("total_strain", k.strain[0]), ("total_flux", k.flux[0])):
            held.one(f"cell {c}", name, v, S[name], y)
        assert k.argmax_element[0] == S["argmax"]
        if labels is not None:
            rec = r.reconstruction
            for name in R.REGION_QUANTITIES + ("mean_strain", "energy", "max_flux"):
                held.one(f"cell {c}", name, getattr(rec, name)[0], S[name], y)
    held.done(f"{shape} state")


# -- the magnitude of the coefficient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NT.MAGNITUDE_SHAPES)
def test_magnitude(shape):
    """coef 2^k, k = +-40, one case per corrector route: the softening law is homogeneous of degree one in c, so after the exact power
    of two A_eff, mean_flux and coef meet the bound of the unscaled case against the unscaled truth, and the strain is unchanged to it."""
    p = _plan(shape)
    law = G.secant_law(NT.soft_law(p.kind, p.dim))
    coef, M, xi = NT.inputs(shape, 0)
    T, y = NT.iteration_reference(shape, 0, 0)
    base = _secant(shape, 0, law, (coef, M, xi), T["rounds"])
    held = Held()
    for k in NT.MAGNITUDE_K:
        r = _secant(shape, 0, law, (coef * 2.0 ** k, M, xi), T["rounds"])
        assert r["info"] == 0 and r["status"] in (0, 1)
        for name in ("A", "mean_flux", "coef", "flux", "values", "strain"):
            v = r[name] if name == "strain" else r[name] * 2.0 ** -k
            held.one(f"2^{k}", name, v.reshape(np.shape(T[name])), T[name], y)
            print(f"{shape} coef 2^{k} {name}: {R.rel(v, base[name]):.2e} from the unscaled device run")
    held.done(f"{shape} magnitude")


# -- the slot path ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eigenstrain", [None, True], ids=["plain", "E"])
def test_slot_path_and_lds_path(eigenstrain):
    """The n = 112 Poisson cell of test_gpu_secant.py::test_slot_path_and_lds_path_on_a_large_cell, one cell, max_iter = 2, tol = 0: the
    deep law puts the field in the slot, the shallow law keeps it in LDS; both against a two-round truth."""
    p = _plan("p2", NT.SLOT_N)
    d = NT.slot_inputs()
    n, deep, shallow = NT.SLOT_N, G.secant_law(NT.deep_law(13)), G.secant_law(NT.deep_law(1))
    # 8 ndof beside fifteen stack rows of 4096 bytes passes the 150 KiB of the round kernel, beside three it does not: two paths
    assert deep.depth == 16 and shallow.depth <= 4 and 8 * n * n + 4096 * 15 > 150 * 1024 >= 8 * n * n + 4096 * 3
    held = Held()
    for levels, name in ((13, "slot"), (1, "lds")):
        T, y = NT.slot_reference(levels, eigenstrain)
        kw = {"P": d["load"], "eigenstrain": True} if eigenstrain else {}
        r = G.secant_outputs(p.secant(d["coef"], d["xi"], G.secant_law(NT.deep_law(levels)), max_iter=2, tol=0.0, fields=True, values=True,
                                      return_coef=True, **kw))
        assert r["rounds"] <= 2  # a float64 change of exactly zero may stop a cell early
        held.arrays(name, r, T, y, ITERATION)
    held.done(f"slot path {'beside an eigenstrain' if eigenstrain else 'plain'}")
