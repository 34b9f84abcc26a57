"""The long-double reference of the nonlinear family (tests/nonlinear_truth.py) checked against itself, and its float64 yardsticks capped
(CPU only; DESIGN 4.11 "Nonlinear outputs").  An ill-posed input must not be able to loosen a bound of
tests/test_gpu_accuracy_nonlinear.py unnoticed: every yardstick of every GPU case is at most 1e-11 (the strain and flux fields and
the history: 1e-10 -- the caps of tests/test_accuracy_ref_host.py for derived quantities and correctors), every contraction factor is
below 0.6, no element sits within 1e-9 of the kink of max(h0, driver) in any round of any load step, every element tangent the sibling
plan eliminates is definite, the largest criterion value leads the second by 1e-9, and no value lies within 1e-9 of the threshold.
"""

import numpy as np
import pytest

import accuracy_gpu as G
import accuracy_ref as R
import nonlinear_truth as NT

LD = R.LD
CAP, CAP_FIELD = 1e-11, 1e-10
FIELD_QUANTITIES = ("strain", "flux", "history", "total_strain", "total_flux")  # the strain and flux fields and the history
WELL = 1e-9


def _capped(what, y, T=None):
    """Every yardstick below its cap; the contraction factor of the truth below 0.6."""
    worst = max(y["e"].values())
    line = f"{what}: worst yardstick {worst:.1e} ({max(y['e'], key=y['e'].get)})"
    if T is not None:
        line += f"; {T['rounds']} rounds, contraction {T['contraction']:.2f}, last change {T['change']:.1e}"
        assert T["contraction"] < 0.6, what
    print(line)
    for name, e in y["e"].items():
        assert e <= (CAP_FIELD if name in FIELD_QUANTITIES else CAP), (what, name, e)
        assert y["bound"][name] == R.FACTOR * max(e, R.FLOOR_EPS * R.EPS)


def _kink_gap(T):
    return min(float((np.abs(d - h) / np.maximum(d, h)).min()) for d, h in T["drivers"])


def _definite(D):
    return float(np.linalg.eigvalsh(D["T"].astype(np.float64)).min())


# -- the module reads the laws and shapes of the coarse tests ---------------------------------------------------------------------------
def test_shapes_and_law_texts_are_those_of_the_coarse_tests():
    import secant_tangent_ref as TR
    import test_gpu_elem_walk_bits as EW
    import test_gpu_secant as GS
    import test_gpu_secant_history as GH

    assert NT.SHAPES == EW.SHAPES
    for shape, (dim, kind, _) in NT.SHAPES.items():
        assert G.secant_law(NT.soft_law(kind, dim)).texts == GS.soft_law(kind, dim).texts
        assert G.secant_law(NT.potential_law(kind, dim)).texts == TR.potential_law(kind, dim)[0].texts
        if shape in NT.HISTORY_SHAPES or shape in NT.STATE_CASES and NT.STATE_CASES[shape][0]:
            a, b = G.secant_law(NT.damage_law(kind, dim)), GH.damage_law(kind, dim)
            assert a.texts == b.texts and a.history_texts == b.history_texts
    assert G.secant_law(NT.potential_law("elasticity", 2, True)).texts == TR.potential_law("elasticity", 2, True)[0].texts
    for kind in ("poisson", "elasticity"):
        a, b = G.secant_law(NT.potential_damage_law(kind, 2)), GH.potential_damage_law(kind, 2)
        assert a.texts == b.texts and a.history_texts == b.history_texts
    assert G.secant_law(NT.deep_law(13)).depth == 16 and G.secant_law(NT.deep_law(1)).depth <= 4


def test_a_long_double_stream_keeps_its_digits():
    c = np.array([LD(1) + LD(2) ** -60, LD(3)])
    assert R.material_tensor("poisson", c, 2)[0, 0, 0] == c[0] and R.material_tensor("poisson", c, 2, np.float64)[0, 0, 0] == 1.0


# -- identity law, closed forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2", "e3"])
def test_identity_law_stops_in_round_one_with_the_numbers_of_derived_truth(shape):
    g = NT.geometry(shape)
    coef, M, xi = NT.inputs(shape, 1)
    n = R.n_components(g["kind"], g["dim"])
    law = NT.Law(g["kind"], g["dim"], [f"c[{k}]" for k in range(n)], lambda e, q, b, h=None: b.copy())
    T = NT.iterate(g, law, coef[0], xi[0], M[0])
    want = R.derived_truth(g["kind"], g["x"], g["cells"], g["tp"], coef[0], M[0], xi=xi[0])
    assert T["rounds"] == 1 and T["change"] == 0.0
    for a, b in (("A", "A"), ("strain", "strain"), ("flux", "flux"), ("mean_flux", "mean_flux")):
        assert np.array_equal(T[a], want[b]), a
    assert np.array_equal(T["coef"], coef[0].astype(LD))


# ten times the measured differences |truth - mpmath| (40 digits): 2.71e-19 (A_H[0][0] = 0.7376), 1.30e-18 (1.2858), 1.84e-18 (1.4901)
LAMINATE_TOL = {None: 10 * 2.71e-19, "P": 10 * 1.30e-18, "E": 10 * 1.84e-18}


@pytest.mark.parametrize("mode", [None, "P", "E"], ids=["plain", "P", "E"])
def test_laminates_against_the_layer_equations_in_mpmath(mode):
    """b = 10 on y0 < 0.25, xi = (2, 0), and the two loaded laminates of test_secant_load_host.layer_value: the
    P1 solution is the layered one, so the truth's fixed point is the root of the two scalar layer equations.  Measured here:
    |A_H[0][0] - mpmath| = 2.71e-19, |mean_flux[0] - mpmath| = 1.30e-18 (P) and 1.84e-18 (E), after 13, 11 and 13 rounds; each tolerance
    is ten times that."""
    g = NT.geometry("p2")
    base, xi, load = NT.laminate()
    T = NT.iterate(g, NT.soft_law("poisson", 2), base, xi, load=load if mode else None, eigenstrain=mode == "E")
    got = T["A"][0, 0] if mode is None else T["mean_flux"][0]
    want = NT.laminate_value(mode)
    print(f"laminate {mode}: {T['rounds']} rounds, truth {got!r}, mpmath {want!r}, difference {float(abs(got - want)):.2e}")
    assert abs(got - want) <= LAMINATE_TOL[mode]
    if mode is None:
        assert abs(float(want) - 0.7375971568657579) <= 1e-15  # the figure DESIGN 4.15 records for the layer equations
        Tl, value, y = NT.laminate_reference()  # what the GPU test reads: the same truth and value, and the float64 yardstick of A_H[0][0]
        assert Tl["A"][0, 0] == got and value == want
        _capped("laminate", y, Tl)
    else:
        from test_secant_load_host import layer_value

        assert abs(float(want) - layer_value(mode == "E")) <= 1e-14


# -- D against Richardson central differences of the truth's own fixed point -------------------------------------------------------------
def _richardson(g, law, coef, xi, M, direction, h, **kw):
    def central(step):
        f = [NT.iterate(g, law, coef, xi + s * step * direction, M, **kw)["mean_flux"] for s in (1.0, -1.0)]
        return (f[0] - f[1]) / (2 * LD(step))

    return (4 * central(h / 2) - central(h)) / 3


# (shape, what) -> |D d - Richardson| / max |D d| measured here with h = 1e-4 (and h / 2), d a seeded direction of largest entry 1.  The
# step is small against the distance of every element from the kink of max(h0, driver) in the frozen case (1.5e-3 relative)
FD_STEP = 1e-4
FD_MEASURED = {("p2", "plain"): 4.43e-13, ("e2", "plain"): 5.59e-13, ("pm3", "plain"): 1.04e-13, ("mesh_ev3", "plain"): 3.12e-13,
               ("p2", "P"): 1.14e-13, ("p2", "E"): 1.70e-13, ("p2", "frozen"): 6.58e-13}


@pytest.mark.parametrize("shape,what", list(FD_MEASURED), ids=[f"{s}-{w}" for s, w in FD_MEASURED])
def test_tangent_against_richardson_differences_of_the_fixed_point(shape, what):
    """The four kinds, a polarisation, an eigenstrain and a frozen history.  D d against (4 C(h/2) - C(h)) / 3, C the central difference
    of the truth's fixed-point mean_flux along a seeded direction d: the agreement reached is asserted to ten times what was measured,
    and nothing above 1e-10 passes.  Measured: 1.0e-13 to 6.6e-13 (FD_MEASURED)."""
    g = NT.geometry(shape)
    kw, hist = {}, None
    if what == "frozen":
        coef, M, xi = (a[0] if a is not None else None for a in NT.inputs(shape, NT.HISTORY_FAMILY))
        law, hist = NT.potential_damage_law(g["kind"], g["dim"]), NT.history_start(shape)[0]
        kw = {"history": hist}
        T, D, _ = NT.frozen_reference(shape, 0)
    elif what == "plain":
        coef, M, xi = (a[0] if a is not None else None for a in NT.inputs(shape, 0, NT.tangent_xi(shape)))
        law = NT.potential_law(g["kind"], g["dim"])
        T, D, _ = NT.tangent_reference(shape, 0, 0)
    else:
        coef, M, xi = (a[0] if a is not None else None for a in NT.inputs(shape, 0, NT.tangent_xi(shape)))
        law = NT.potential_law(g["kind"], g["dim"])
        kw = {"load": NT.load_of(shape, 0)[0], "eigenstrain": what == "E"}
        T, D, _ = NT.load_reference(shape, 0, what == "E")
    d = np.random.default_rng(R.case_seed("fd direction", shape, what)).standard_normal(g["t"])
    d /= np.abs(d).max()
    fd = _richardson(g, law, coef, xi, M, d, FD_STEP, **kw)
    want = D["D"] @ d.astype(LD)
    err = float(np.abs(want - fd).max() / np.abs(want).max())
    print(f"{shape} {what}: |D d - Richardson| = {err:.2e} of the largest entry; asymmetry {D['asymmetry']:.1e}; D against A {R.rel(D['D'], T['A']):.3f}")
    assert D["asymmetry"] <= 64 * NT.EPS_LD  # a potential: D is the derivative itself
    assert R.rel(D["D"], T["A"]) > 0.01  # and it is not the secant tensor
    assert err <= 1e-10
    assert FD_MEASURED[(shape, what)] is not None and err <= 10 * FD_MEASURED[(shape, what)]


# -- the yardsticks of every GPU case, and what makes its comparisons well-posed --------------------------------------------------------------
@pytest.mark.parametrize("shape,fi", NT.ITERATION_CASES, ids=[f"{s}-{NT.FAMILY_IDS[fi]}" for s, fi in NT.ITERATION_CASES])
def test_iteration_cases(shape, fi):
    for c in range(NT.NC):
        for relax in NT.RELAX:
            T, y = NT.iteration_reference(shape, fi, c, relax, 4)
            assert T["rounds"] == 4
            _capped(f"{shape} {NT.FAMILY_IDS[fi]} cell {c} relax {relax} round 4", y)
    for c in range(NT.cells_of(shape)):
        T, y = NT.iteration_reference(shape, fi, c)
        _capped(f"{shape} {NT.FAMILY_IDS[fi]} cell {c} fixed point", y, T)
        assert T["change"] <= 1e-16  # the remainder of the truth, change L / (1 - L), is far below every bound (1.1e-13 at least)


@pytest.mark.parametrize("shape", NT.MAGNITUDE_SHAPES)
def test_the_softening_law_is_homogeneous_of_degree_one(shape):
    """coef 2^k: the truth's fixed point scales exactly -- A, mean_flux and coef by 2^k, the strain not at all (a power of two commutes
    with every rounding), so the GPU test may hold the scaled device run against the unscaled truth."""
    g, coef, M, xi = NT._cell(shape, 0, 0)
    law = NT.soft_law(g["kind"], g["dim"])
    T = NT.iteration_reference(shape, 0, 0)[0]
    for k in NT.MAGNITUDE_K:
        S = NT.iterate(g, law, coef * 2.0 ** k, xi, M)
        assert S["rounds"] == T["rounds"] and np.array_equal(S["strain"], T["strain"])
        for name in ("A", "mean_flux", "coef"):
            assert np.array_equal(S[name] * LD(2) ** -k, T[name]), (name, k)


@pytest.mark.parametrize("shape,fi", NT.TANGENT_CASES, ids=[f"{s}-{NT.FAMILY_IDS[fi]}" for s, fi in NT.TANGENT_CASES])
def test_tangent_cases(shape, fi):
    for c in range(NT.cells_of(shape)):
        T, D, y = NT.tangent_reference(shape, fi, c)
        _capped(f"tangent {shape} {NT.FAMILY_IDS[fi]} cell {c}", y, T)
        print(f"  smallest eigenvalue of an element tangent {_definite(D):.2e}; D against A {R.rel(D['D'], T['A']):.3f}")
        assert _definite(D) > 0 and D["asymmetry"] <= 64 * NT.EPS_LD and "asymmetry" not in y["e"]


def test_asymmetric_case():
    shape, fi = NT.ASYMMETRIC_CASE
    for c in range(NT.NC):
        T, D, y = NT.tangent_reference(shape, fi, c, True)
        _capped(f"asymmetric {shape} cell {c}", y, T)
        assert D["asymmetry"] > 1e-3 and "asymmetry" in y["e"] and _definite(D) > 0


@pytest.mark.parametrize("shape", NT.LOAD_SHAPES)
def test_load_cases(shape):
    for c in range(NT.cells_of(shape)):
        for eig in (False, True):
            T, D, y = NT.load_reference(shape, c, eig)
            _capped(f"load {shape} cell {c} {'E' if eig else 'P'}", y, T)
            assert _definite(D) > 0 and D["asymmetry"] <= 64 * NT.EPS_LD
            plain = NT.tangent_reference(shape, 0, c)[0]
            assert R.rel(T["mean_flux"], plain["mean_flux"]) > 0.01  # the load matters


@pytest.mark.parametrize("shape", NT.HISTORY_SHAPES)
def test_history_cases(shape):
    """Load, increase, unload: the kink of max(h0, driver) in every round of every step; unloading: D is A_eff of the damaged stream and
    no history value grows (not a bit)."""
    for c in range(NT.NC):
        steps = NT.history_reference(shape, c)
        h = np.zeros_like(steps[0][0]["history"])
        for k, (T, D, y) in enumerate(steps):
            _capped(f"history {shape} cell {c} step {k}", y, T)
            gap = _kink_gap(T)
            loading = [float((d > h0).mean()) for d, h0 in T["drivers"]][-1]
            print(f"  kink gap {gap:.1e}, loading elements {loading:.2f}, smallest eigenvalue of an element tangent {_definite(D):.2e}")
            assert gap >= WELL and _definite(D) > 0
            assert (T["history"] >= h).all()
            if k < 2:
                assert (T["history"] > h).any() and loading > 0.5
            else:
                assert T["rounds"] == 2 and loading == 0.0 and np.array_equal(T["history"], h)
                assert R.rel(D["D"], T["A"]) <= 16 * NT.EPS_LD and D["asymmetry"] == 0.0
            h = T["history"]


@pytest.mark.parametrize("shape", NT.HISTORY_TANGENT_SHAPES)
def test_frozen_history_cases(shape):
    for c in range(NT.NC):
        T, D, y = NT.frozen_reference(shape, c)
        _capped(f"frozen {shape} cell {c}", y, T)
        d, h0 = T["drivers"][-1]
        print(f"  kink gap {_kink_gap(T):.1e}, loading elements {float((d > h0).mean()):.2f}")
        assert _kink_gap(T) >= WELL and (d > h0).any() and (d < h0).any()  # both branches of max
        assert _definite(D) > 0 and D["asymmetry"] <= 64 * NT.EPS_LD


@pytest.mark.parametrize("shape", list(NT.STATE_CASES))
def test_state_cases(shape):
    crit = NT.state_case(shape)[1]
    for c in range(NT.NC):
        T, S, y = NT.state_reference(shape, c)
        _capped(f"state {shape} cell {c}", y, T)
        v = np.sort(S["crit_values"])
        lead = float((v[-1] - v[-2]) / v[-1])
        near = float(np.abs(v / LD(crit.threshold) - 1).min())
        frac = float(S["exceed_volume"])
        print(f"  argmax leads by {lead:.1e}; nearest value to the threshold {near:.1e}; exceed volume {frac:.3f}")
        assert lead >= WELL and near >= WELL and 0.1 < frac < 0.9
        if T["drivers"]:
            assert _kink_gap(T) >= WELL
        if shape == "pm3":
            assert (S["region_volume"] > 0).all() and len(S["region_volume"]) == 2


@pytest.mark.parametrize("levels", [13, 1], ids=["slot", "lds"])
def test_slot_cases(levels):
    for eig in (None, True):
        T, y = NT.slot_reference(levels, eig)
        assert T["rounds"] == 2
        _capped(f"slot levels {levels} {'E' if eig else 'plain'}", y)
