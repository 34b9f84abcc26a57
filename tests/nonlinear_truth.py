"""Extended-precision reference of the nonlinear family (NumPy ``longdouble``; no GPU; DESIGN 4.11 "Nonlinear outputs"): the secant
iteration, its consistent tangent, history variables, a load beside the law, criteria and region rows of the stopped state -- one cell at a
time, by the rules of include/hommx_hip.h and the docstrings of secant_ref, history_ref, secant_load_ref, secant_tangent_ref and
secant_state_ref, on the long-double cell problems of ``accuracy_ref.derived_truth``.

The laws are plain NumPy formulas on arrays of either number format, written beside the text ``SecantLaw`` / ``Criterion`` gets for the
same law: a second, independent reading.  The module imports accuracy_ref and nothing of hommx_amd: the ``SecantLaw`` / ``Criterion`` of a law's texts
is made by ``accuracy_gpu.secant_law`` / ``accuracy_gpu.criterion``, for the device and for the float64 references.  Nothing of ``host_values``,
``host_tangent`` or ``_run`` is used by the truth; the float64
references of the coarse tests, which do use them, are run by ``float64_errors`` alone -- their errors against the truth are the
yardsticks of tests/test_gpu_accuracy_nonlinear.py:

    e_gpu <= accuracy_ref.FACTOR * max(e_float64, accuracy_ref.FLOOR_EPS * eps)        (``accuracy_ref.bound``; never from a device result).

A decimal constant of a law's text (0.7) is the float64 the parser makes of it, on both sides: a Python float times a long-double
array converts exactly.  The iterates of the truth are long double (``accuracy_ref.material_tensor`` keeps them), the device commits
float64: one rounding per round, which the contraction of the map keeps at the size of one.

The case tables and seeds of the host test and the GPU test live at the end.
"""

from __future__ import annotations

import functools

import numpy as np

import accuracy_ref as R

LD = R.LD
EPS_LD = float(np.finfo(LD).eps)
VOIGT_DIAGONAL = (0, 6, 11, 15, 18, 20)  # of the 21 entries, the upper triangle of the 6 x 6 tensor row by row
TANGENT_KIND = {"poisson": "poisson_matrix", "poisson_matrix": "poisson_matrix", "elasticity": "elasticity_voigt",
                "elasticity_voigt": "elasticity_voigt"}


# ------------------------------------------------------------------------------------------------------------------------------
# the laws: text for the library, formula for the truth
# ------------------------------------------------------------------------------------------------------------------------------


class Law:
    """texts[n_comp] (and the texts of the history updates) as the library parses them, and the same law as formulas on arrays
    e[n_el, t] (doubled shear), q[n_el, t], b[n_el, n_comp], h[n_el, n_history] of one number format:
    values -> v[n_el, n_comp];  updates -> h'[n_el, n_history] or None;  dlaw -> dv/de[n_el, n_comp, t] at frozen h;
    drivers -> (driver[n_el], h0[n_el]) of the law's max(h0, driver), or None."""

    def __init__(self, kind, dim, texts, values, dlaw=None, history_texts=None, updates=None, drivers=None):
        self.kind, self.dim, self.texts, self.values, self.dlaw = kind, dim, list(texts), values, dlaw
        self.history_texts, self.updates, self.drivers = history_texts, updates, drivers
        self.n_history = 0 if history_texts is None else len(history_texts)
        self.potential = None  # (kind, dim, asymmetric) of a law secant_tangent_ref.potential_law writes down with its derivative


def _zeros(e, n):
    return np.zeros((e.shape[0], n, e.shape[1]), dtype=e.dtype)


def soft_law(kind, dim) -> Law:
    """The softening law of tests/test_gpu_secant.py: every entry of the base times 0.5 + 0.5 / (1 + e0^2 + e1^2); of the 21 Voigt
    entries the six diagonal ones times 1 + 0.5 / (1 + e0^2), the others copied.  Homogeneous of degree one in the base."""
    n = R.n_components(kind, dim)
    if n == 21:
        diag = list(VOIGT_DIAGONAL)
        texts = [f"c[{k}]*(1 + 0.5/(1 + e[0]**2))" if k in diag else f"c[{k}]" for k in range(n)]

        def values(e, q, b, h=None):
            v = b.copy()
            v[:, diag] = b[:, diag] * (1 + 0.5 / (1 + e[:, 0] ** 2))[:, None]
            return v

        def dlaw(e, b, h=None):
            d = _zeros(e, n)
            d[:, diag, 0] = b[:, diag] * (-e[:, 0] / (1 + e[:, 0] ** 2) ** 2)[:, None]
            return d

        return Law(kind, dim, texts, values, dlaw)
    texts = [f"c[{k}]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))" for k in range(n)]

    def values(e, q, b, h=None):
        return b * (0.5 + 0.5 / (1 + e[:, 0] ** 2 + e[:, 1] ** 2))[:, None]

    def dlaw(e, b, h=None):
        d = _zeros(e, n)
        g = 1 + e[:, 0] ** 2 + e[:, 1] ** 2
        for j in (0, 1):
            d[:, :, j] = b * (-e[:, j] / g ** 2)[:, None]
        return d

    return Law(kind, dim, texts, values, dlaw)


def _voigt_entries(t):
    return [(m, n) for m in range(t) for n in range(m, t)]


def potential_law(kind, dim, asymmetric=False) -> Law:
    law = _potential_law(kind, dim, asymmetric)
    law.potential = (kind, dim, asymmetric)
    return law


def _potential_law(kind, dim, asymmetric) -> Law:
    """The potential laws of tests/secant_tangent_ref.py (phi(s) = 0.5 + 0.5 / (1 + s), psi(s) = 0.5 / (1 + s)):
    poisson c0 phi(|e|^2); poisson_matrix the diagonal entries c[k] + psi(|e|^2); elasticity lam = c0, mu = c1 phi(eps : eps) with
    eps : eps = sum normal^2 + 0.5 sum shear^2; elasticity_voigt the diagonal entry of row r is c[k] + 0.5 / (1 + e[r]^2).
    ``asymmetric``: the mu law with the shear term counted twice as much -- no potential."""
    t, n = R.tensor_size(kind, dim), R.n_components(kind, dim)
    if kind == "poisson":
        s = " + ".join(f"e[{i}]**2" for i in range(t))

        def values(e, q, b, h=None):
            return b * (0.5 + 0.5 / (1 + (e ** 2).sum(axis=1)))[:, None]

        def dlaw(e, b, h=None):
            return (b[:, 0, None] * (-e / (1 + (e ** 2).sum(axis=1))[:, None] ** 2))[:, None, :]

        return Law(kind, dim, [f"c[0]*(0.5 + 0.5/(1 + {s}))"], values, dlaw)
    if kind == "poisson_matrix":
        s = " + ".join(f"e[{i}]**2" for i in range(t))
        texts = [f"c[{k}] + 0.5/(1 + {s})" if k < dim else f"c[{k}]" for k in range(n)]  # the ABI lists the diagonal first

        def values(e, q, b, h=None):
            v = b.copy()
            v[:, :dim] += (0.5 / (1 + (e ** 2).sum(axis=1)))[:, None]
            return v

        def dlaw(e, b, h=None):
            d = _zeros(e, n)
            d[:, :dim, :] = (-e / (1 + (e ** 2).sum(axis=1))[:, None] ** 2)[:, None, :]
            return d

        return Law(kind, dim, texts, values, dlaw)
    if kind == "elasticity":
        w = np.array([1.0] * dim + [1.0 if asymmetric else 0.5] * (t - dim))
        s = " + ".join([f"e[{i}]**2" for i in range(dim)] + [(f"e[{i}]**2" if asymmetric else f"0.5*e[{i}]**2") for i in range(dim, t)])

        def values(e, q, b, h=None):
            v = b.copy()
            v[:, 1] = b[:, 1] * (0.5 + 0.5 / (1 + (w.astype(e.dtype) * e ** 2).sum(axis=1)))
            return v

        def dlaw(e, b, h=None):
            d = _zeros(e, 2)
            ww = w.astype(e.dtype)
            d[:, 1, :] = b[:, 1, None] * (-ww * e / (1 + (ww * e ** 2).sum(axis=1))[:, None] ** 2)
            return d

        return Law(kind, dim, ["c[0]", f"c[1]*(0.5 + 0.5/(1 + {s}))"], values, dlaw)
    ent = _voigt_entries(t)
    rows = [(k, r) for k, (r, c) in enumerate(ent) if r == c]
    texts = [f"c[{k}] + 0.5/(1 + e[{r}]**2)" if r == c else f"c[{k}]" for k, (r, c) in enumerate(ent)]

    def values(e, q, b, h=None):
        v = b.copy()
        for k, r in rows:
            v[:, k] = b[:, k] + 0.5 / (1 + e[:, r] ** 2)
        return v

    def dlaw(e, b, h=None):
        d = _zeros(e, n)
        for k, r in rows:
            d[:, k, r] = -e[:, r] / (1 + e[:, r] ** 2) ** 2
        return d

    return Law(kind, dim, texts, values, dlaw)


def _damage(kind, dim, driver_text, driver, ddriver) -> Law:
    """Every entry of the base times g(kappa) = 1 - 0.5 (1 - exp(-kappa / 0.7)), kappa = max(h0, driver(e, b)); the update is kappa."""
    n = R.n_components(kind, dim)
    kappa = f"max(h[0], {driver_text})"
    texts = [f"c[{k}]*(1 - 0.5*(1 - exp(-{kappa}/0.7)))" for k in range(n)]

    def g(k):
        return 1 - 0.5 * (1 - np.exp(-k / 0.7))

    def values(e, q, b, h):
        return b * g(np.maximum(h[:, 0], driver(e, b)))[:, None]

    def updates(e, q, b, h):
        return np.maximum(h[:, 0], driver(e, b))[:, None]

    def dlaw(e, b, h):
        dr = driver(e, b)
        k = np.maximum(h[:, 0], dr)
        dg = np.where(dr > h[:, 0], -0.5 / 0.7 * np.exp(-k / 0.7), 0 * k)  # an element that does not load has no tangent term
        return b[:, :, None] * (dg[:, None] * ddriver(e, b, dr))[:, None, :]

    return Law(kind, dim, texts, values, dlaw, [kappa], updates, lambda e, b, h: (driver(e, b), h[:, 0]))


def damage_law(kind, dim) -> Law:
    """The damage law of tests/test_gpu_secant_history.py: kappa = max(h0, sqrt(e0^2 + e1^2))."""
    def driver(e, b):
        return np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)

    def ddriver(e, b, dr):
        d = np.zeros_like(e)
        d[:, :2] = e[:, :2] / dr[:, None]
        return d

    return _damage(kind, dim, "sqrt(e[0]**2 + e[1]**2)", driver, ddriver)


def potential_damage_law(kind, dim) -> Law:
    """``potential_damage_law`` of the same file: the driver is the energy norm of the BASE tensor where |e| is none -- 2D Lame:
    sqrt(c0 (e0 + e1)^2 + 2 c1 (e0^2 + e1^2) + c1 e2^2) --, so that the derivative of the stress is symmetric."""
    if kind == "poisson":
        return damage_law(kind, dim)
    assert kind == "elasticity" and dim == 2

    def driver(e, b):
        return np.sqrt(b[:, 0] * (e[:, 0] + e[:, 1]) ** 2 + 2 * b[:, 1] * (e[:, 0] ** 2 + e[:, 1] ** 2) + b[:, 1] * e[:, 2] ** 2)

    def ddriver(e, b, dr):
        tr = b[:, 0] * (e[:, 0] + e[:, 1])
        return np.stack([tr + 2 * b[:, 1] * e[:, 0], tr + 2 * b[:, 1] * e[:, 1], b[:, 1] * e[:, 2]], axis=1) / dr[:, None]

    return _damage(kind, dim, "sqrt(c[0]*(e[0] + e[1])**2 + 2*c[1]*(e[0]**2 + e[1]**2) + c[1]*e[2]**2)", driver, ddriver)


def deep_law(levels: int = 13) -> Law:
    """The scalar laws of the slot test of tests/test_gpu_secant.py: c0 / (1 + (1 + ... (1 + e0^2))) with ``levels`` additions
    (13: depth 16, the field in the slot; 1: the shallow law, the field in LDS)."""
    text = "e[0]**2"
    for _ in range(levels):
        text = f"(1 + {text})"
    return Law("poisson", 2, [f"c[0]/{text}"], lambda e, q, b, h=None: _deep(e, b, levels))


def _deep(e, b, levels):
    v = e[:, 0] ** 2
    for _ in range(levels):  # the additions one by one, as the program makes them (the sums are exact in long double for all that matters)
        v = 1 + v
    return b / v[:, None]


class Crit:
    """The criterion of the state tests: the flux norm over the base coefficient, weighted by the strain and, for a law with a history
    variable, by the history: sqrt(s0^2 + s1^2) / b0 * (1 + abs(e0)) [/ (1 + h0)].  It reads e, s, b[k] and h[k]."""

    def __init__(self, with_history: bool, threshold: float):
        self.with_history, self.threshold = with_history, threshold
        self.text = "sqrt(s[0]**2 + s[1]**2)/b[0]*(1 + abs(e[0]))" + ("/(1 + h[0])" if with_history else "")

    def values(self, e, q, b, h=None):
        v = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) / b[:, 0] * (1 + np.abs(e[:, 0]))
        return v / (1 + h[:, 0]) if self.with_history else v


# ------------------------------------------------------------------------------------------------------------------------------
# the truth
# ------------------------------------------------------------------------------------------------------------------------------


def _round(g, kind, c, shape, M, xi, load, eigenstrain):
    """What one round sees on the long-double stream c[n_el, n_comp]: the total strain ``e`` and flux ``q`` = material(c) e + P (P the
    polarisation or the eigenstress -material(c) E of THIS stream), the strain ``s`` the law reads (total, or elastic e - E), A, vol."""
    dim = g["dim"]
    P = None
    if load is not None:
        E = np.asarray(load).astype(LD)
        P = -np.einsum("etu,eu->et", R.voigt_material(kind, c.reshape(shape), dim), E) if eigenstrain else E
    T = R.derived_truth(kind, g["x"], g["cells"], g["tp"], c.reshape(shape), M, xi=xi, loads=None if P is None else P[None])
    e, q = T["strain"], T["flux"]
    if P is not None:
        e, q = e + T["load_strain"][0], q + T["load_flux"][0]
    s = e - E if (P is not None and eigenstrain) else e
    return {"A": T["A"], "e": e, "q": q, "s": s, "vol": T["vol"], "mean_flux": T["vol"] @ q}


def iterate(g, law: Law, base, xi, M=None, load=None, eigenstrain=False, history=None, relax=1.0, coef_start=None, rounds=None,
            max_rounds=120) -> dict:
    """The iteration of one cell in long double, with the round structure of ``secant_load_ref.iterate``.  ``g``: ``geometry(shape)``.
    ``rounds``: that many rounds exactly; None: to the fixed point -- until the change is at most 4 eps_ld or does not decrease any more.
    Returns the state of the stopping round as the device does: ``A``, ``mean_flux``, ``coef`` (the stream that round read), ``strain``
    and ``flux`` (what the law read), ``values`` (what it gave), ``history``, ``change``, ``rounds``; also ``changes``, ``contraction``
    (the largest ratio of successive changes above 1e-15, where rounding has no part), ``total_strain``, ``total_flux``, ``vol`` and
    ``drivers``, the (driver, h0) of every round of a law with max(h0, driver)."""
    kind = law.kind
    base = np.asarray(base, dtype=np.float64)
    n_el = base.shape[0]
    b = base.reshape(n_el, -1).astype(LD)
    c = b.copy() if coef_start is None else np.asarray(coef_start).astype(LD).reshape(n_el, -1)
    h = None if history is None else np.asarray(history).astype(LD).reshape(n_el, law.n_history)
    changes, drivers = [], []
    j = 0
    while True:
        st = _round(g, kind, c, base.shape, M, xi, load, eigenstrain)
        v = law.values(st["s"], st["q"], b, h)
        if law.drivers is not None:
            drivers.append(law.drivers(st["s"], b, h))
        w = v if relax == 1.0 else (1 - LD(relax)) * c + LD(relax) * v
        top, diff = np.abs(w).max(), np.abs(w - c).max()
        change = LD(0) if top == 0 and diff == 0 else diff / top
        changes.append(float(change))
        j += 1
        if rounds is not None:
            if j == rounds:
                break
        elif change <= 4 * EPS_LD or (j > 2 and changes[-1] >= changes[-2]) or j == max_rounds:
            break
        c = w
    ratios = [changes[k + 1] / changes[k] for k in range(len(changes) - 1) if changes[k + 1] > 1e-15]
    out = {"A": st["A"], "mean_flux": st["mean_flux"], "coef": c.reshape(base.shape), "strain": st["s"], "flux": st["q"],
           "values": v, "history": None if h is None else law.updates(st["s"], st["q"], b, h), "change": changes[-1], "rounds": j,
           "changes": changes, "contraction": max(ratios) if ratios else 0.0, "total_strain": st["e"], "total_flux": st["q"],
           "vol": st["vol"], "drivers": drivers, "flux_weights": g["flux_weights"]}
    return out


def tangent_stream(kind, dim, T):
    """The symmetric T[n_el, t, t] as an element stream of the tangent kind, in the order of the ABI."""
    ent = R.PAIRS[dim] if kind.startswith("poisson") else _voigt_entries(T.shape[1])
    return np.stack([T[:, r, c] for r, c in ent], axis=-1)


def tangent(g, law: Law, r: dict, base, M=None, history=None) -> dict:
    """The consistent tangent at the state ``r`` of ``iterate``, in long double:
    T_K = material(c_K) + sum_k (material(unit_k) e_K) (dL_k/de)^T  at the strain the law saw and at frozen history; ``asymmetry`` =
    max |T - T^T| / max |T|; ``tangent_coef`` the stream of the symmetric part; ``D`` = A_eff of that stream on the tangent kind."""
    kind, dim = law.kind, g["dim"]
    base = np.asarray(base, dtype=np.float64)
    n_el = base.shape[0]
    b = base.reshape(n_el, -1).astype(LD)
    n = b.shape[1]
    h = None if history is None else np.asarray(history).astype(LD).reshape(n_el, law.n_history)
    e = r["strain"]
    T = R.voigt_material(kind, r["coef"], dim).copy()
    dc = law.dlaw(e, b, h)
    for k in range(n):
        unit = np.zeros((1, n))
        unit[0, k] = 1.0
        U = R.voigt_material(kind, unit.reshape((1,) + base.shape[1:]), dim)[0]
        T += np.einsum("mn,en->em", U, e)[:, :, None] * dc[:, k, None, :]
    top = np.abs(T).max()
    sym = (T + np.transpose(T, (0, 2, 1))) / 2
    stream = tangent_stream(kind, dim, sym)
    D = R.truth(TANGENT_KIND[kind], g["x"], g["cells"], g["tp"], stream, M)[0]
    return {"T": sym, "tangent_coef": stream, "asymmetry": float(np.abs(T - np.transpose(T, (0, 2, 1))).max() / top), "D": D}


def state(r: dict, crit: Crit, base, history=None, labels=None, n_regions=0) -> dict:
    """On the state ``r`` of ``iterate``: the criterion's ``values``, ``max``, ``argmax``, ``mean`` (sum |K| v_K) and ``exceed_volume``
    (the volume of v_K >= threshold) on the TOTAL strain and flux, the stream of the stopping round, the base and the history of the
    start of the call; with ``labels`` the region rows of ``accuracy_ref.region_rows`` on the total fields."""
    base = np.asarray(base, dtype=np.float64)
    b = base.reshape(base.shape[0], -1).astype(LD)
    e, q, vol = r["total_strain"], r["total_flux"], r["vol"]
    out = {"total_strain": e, "total_flux": q}
    h = None if history is None else np.asarray(history).astype(LD).reshape(base.shape[0], -1)
    v = crit.values(e, q, b, h)
    out.update(crit_values=v, max=v.max(), argmax=int(np.argmax(v)), mean=vol @ v, exceed_volume=vol[v >= crit.threshold].sum())
    if labels is not None:
        w = np.asarray(r["flux_weights"]).astype(LD)
        nrm = np.sqrt(np.einsum("t,et->e", w, q * q))
        out.update(R.region_rows(vol, e, q, nrm, labels, n_regions))
        out.update(mean_strain=vol @ e, energy=vol @ np.einsum("et,et->e", e, q), max_flux=nrm.max())
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 yardsticks
# ------------------------------------------------------------------------------------------------------------------------------


def _ref_kw(g):
    return {"n": g["n"]} if g["n"] else {"msh": g["msh"]}


def float64_errors(g, law: Law, base, xi, M, T: dict, load=None, eigenstrain=False, history=None, relax=1.0, with_tangent: dict | None = None,
                   with_state: dict | None = None, crit: Crit | None = None, labels=None, n_regions=0) -> dict:
    """The matching float64 reference of the coarse tests on the same inputs, ``T["rounds"]`` rounds at tol = 0 -- secant_ref (plain),
    history_ref (a history), secant_load_ref (a load, or a state tail: a zero polarisation without a load, as secant_state_ref) --,
    and per quantity its error against the truth ``T`` of ``iterate``, relative to the largest entry of the truth (``accuracy_ref.rel``):
    {"e": {name: e}, "bound": {name: accuracy_ref.bound(e, 0)}, "history64": the reference's own history output or None}.  ``with_tangent``: the result of ``tangent`` -- D, tangent_coef and the
    asymmetry of secant_tangent_ref / secant_load_ref.tangent (their element tangent with this module's derivative evaluated in float64
    for a law with history, for which secant_tangent_ref writes none down).  ``with_state``: the result of ``state`` (with ``crit``) -- the values and
    statistics of secant_state_ref, the region rows of accuracy_ref.region_rows on its fields."""
    import accuracy_gpu as G
    import history_ref as HR
    import secant_load_ref as SL
    import secant_ref as S
    import secant_state_ref as ST
    import secant_tangent_ref as TR

    kind, dim = law.kind, g["dim"]
    law64 = G.secant_law(law)
    kw = dict(max_iter=T["rounds"], tol=0.0, relax=relax)
    base = np.asarray(base, dtype=np.float64)
    n_el = base.shape[0]
    b = base.reshape(n_el, -1)
    h = None if history is None else np.asarray(history, dtype=np.float64).reshape(n_el, law.n_history)
    e = {}
    if with_state is not None:
        r = ST.evaluate(SL.cells(kind, dim, **_ref_kw(g)), law64, G.criterion(crit), base, xi, load, eigenstrain, M, history=h, **kw)
    elif load is not None:
        r = SL.iterate(SL.cells(kind, dim, **_ref_kw(g)), law64, base, xi, load, eigenstrain, M, history=h, **kw)
    elif h is not None:
        r = HR.iterate(HR.solver(kind, dim, **_ref_kw(g)), law64, base, xi, h, M, **kw)
    else:
        r = S.iterate(S.solver(kind, dim, **_ref_kw(g)), law64, base, xi, M, **kw)
    assert r["status"] in (0, 1), r["status"]
    hk = {} if h is None else {"history": h[None]}
    vals = law64.host_values(r["s"][None], r["q"][None], b[None], np.zeros((1, 3)), None, None, **hk)[0]
    for name, got in (("coef", r["coef"]), ("A", r["A"]), ("mean_flux", r["mean_flux"]), ("strain", r["s"]), ("flux", r["q"]),
                      ("values", vals)):
        e[name] = R.rel(got, T[name])
    if h is not None:
        e["history"] = R.rel(r["history"], T["history"])
    if with_tangent is not None:
        dlaw64 = lambda s, bb: law.dlaw(s, bb, h)  # noqa: E731  (the same formula in float64; the potential laws have TR's own below)
        if law.potential is not None:
            dlaw64 = TR.potential_law(*law.potential)[1]
        Tk = TR.element_tangent(kind, dim, r["s"], r["coef"], base, dlaw64)
        top = np.abs(Tk).max()
        sym = 0.5 * (Tk + Tk.transpose(0, 2, 1))
        stream = TR.tangent_stream(kind, dim, sym)
        D = SL.cells(TR.TANGENT_KIND[kind], dim, **_ref_kw(g))(stream, M).A
        e["D"], e["tangent_coef"] = R.rel(D, with_tangent["D"]), R.rel(stream, with_tangent["tangent_coef"])
        if with_tangent["asymmetry"] > 1e-3:  # a law without a potential: the asymmetry is a number to compare
            e["asymmetry"] = R.rel(np.abs(Tk - Tk.transpose(0, 2, 1)).max() / top, with_tangent["asymmetry"])
    if with_state is not None:
        W = with_state
        for name, got in (("crit_values", r["values"]), ("max", r["max"]), ("mean", r["mean"]), ("exceed_volume", r["exceed_volume"]),
                          ("total_strain", r["total_strain"]), ("total_flux", r["total_flux"])):
            e[name] = R.rel(got, W[name])
        if labels is not None:
            q64 = r["total_flux"]
            nrm = np.sqrt(np.einsum("t,et->e", np.asarray(T["flux_weights"], dtype=np.float64), q64 * q64))
            vol = r["cell"].vol
            rows = R.region_rows(vol, r["total_strain"], q64, nrm, labels, n_regions)
            rows.update(mean_strain=vol @ r["total_strain"], energy=vol @ np.einsum("et,et->e", r["total_strain"], q64), max_flux=nrm.max())
            for name in R.REGION_QUANTITIES + ("mean_strain", "energy", "max_flux"):
                e[name] = R.rel(rows[name], W[name])
    return {"e": e, "bound": {k: R.bound(v, 0.0) for k, v in e.items()}, "history64": r["history"] if h is not None else None}


# ------------------------------------------------------------------------------------------------------------------------------
# geometries, inputs and case tables of tests/test_nonlinear_truth_host.py and tests/test_gpu_accuracy_nonlinear.py
# ------------------------------------------------------------------------------------------------------------------------------

NC = 2
SHAPES = {  # those of tests/test_gpu_elem_walk_bits.py: name -> (dim, kind, n or None for the jittered mesh of that dimension)
    "p2": (2, "poisson", 8), "e2": (2, "elasticity", 5), "pm3": (3, "poisson_matrix", 3), "e3": (3, "elasticity", 3),
    "mesh_p2": (2, "poisson", None), "mesh_ev3": (3, "elasticity_voigt", None),
}
MESHES = {2: ("jittered_unit_square", (9, 7)), 3: ("jittered_unit_cube", (3, 4, 3))}
# (coefficient family or None for the kind's top-contrast family, M family or None)
FAMILIES = (("log2", None), (None, "mild"), ("log2", "shear30"))
FAMILY_IDS = ("log2-noM", "top-mild", "log2-shear30")


@functools.lru_cache(maxsize=None)
def geometry(shape, n=None) -> dict:
    """x, cells, tp (the periodic node of every vertex) of a shape, and what the float64 references take: ``n`` or ``msh``."""
    dim, kind, n0 = SHAPES[shape]
    n = n or n0
    if n:
        x, cells, tp = R.structured(dim, n)
        msh = None
    else:
        msh = R.mesh_of(*MESHES[dim])
        x, cells, tp = R.mesh_arrays(msh)
    t = R.tensor_size(kind, dim)
    return {"x": x, "cells": np.asarray(cells), "tp": tp, "n": n, "msh": msh, "dim": dim, "kind": kind, "t": t, "n_el": len(cells),
            "flux_weights": np.array([1.0 if (kind.startswith("poisson") or m < dim) else 2.0 for m in range(t)])}


@functools.lru_cache(maxsize=None)
def inputs(shape, fi, xi_scale=1.0):
    """(coef[NC, n_el(, n_comp)], M[NC, d, d] or None, xi[NC, t]) of a shape and family: the coefficient and M of accuracy_ref's families,
    seeded by the case; the macro strain standard normal times ``xi_scale``.  Read only."""
    dim, kind, _ = SHAPES[shape]
    g = geometry(shape)
    family, mf = FAMILIES[fi]
    family = family or R.top_family(kind)
    seed = R.case_seed("nonlinear", shape, family, mf)
    coef = R.coefficients(kind, dim, g["n_el"], family, NC, seed)
    M = None if mf is None else R.stratification_family(mf, dim, NC, seed)
    xi = xi_scale * np.random.default_rng(seed + 1).standard_normal((NC, g["t"]))
    for a in (coef, M, xi):
        if a is not None:
            a.setflags(write=False)
    return coef, M, xi


def load_of(shape, fi):
    """One seeded load per cell, of order 0.3 with a non-zero mean (the recipe of tests/test_gpu_secant_load.py ``_load``)."""
    g = geometry(shape)
    rng = np.random.default_rng(R.case_seed("nonlinear load", shape, fi))
    return 0.3 * rng.standard_normal((NC, g["n_el"], g["t"])) + 0.2 * rng.standard_normal((NC, 1, g["t"]))


def labels_of(shape):
    """Two regions, both occupied."""
    g = geometry(shape)
    lab = (np.random.default_rng(R.case_seed("nonlinear labels", shape)).random(g["n_el"]) < 0.4).astype(np.uint8)
    lab[:2] = (0, 1)
    return lab


def laminate():
    """The laminate of DESIGN 4.15 on ``p2``: b = 10 on y0 < 0.25, else 1; xi = (2, 0); and the load of the two loaded laminates of
    DESIGN 4.18 (tests/test_secant_load_host.py): 0.5 in the stiff layer, -0.2 in the other, first entry."""
    g = geometry("p2")
    stiff = g["x"][g["cells"]].mean(axis=1)[:, 0] < 0.25
    base = np.where(stiff, 10.0, 1.0)
    load = np.stack([np.where(stiff, 0.5, -0.2), np.zeros(g["n_el"])], axis=-1)
    return base, np.array([2.0, 0.0]), load


def laminate_value(mode: str | None, digits: int = 40):
    """The closed form of the laminates from the scalar layer equations, solved with mpmath to ``digits``: the normal flux is constant
    and the total strains of the layers average to 2.  mode None: A_H[0][0] = q / 2; "P" / "E": mean_flux[0] = q beside the
    polarisation / the eigenstrain."""
    import mpmath as mp

    with mp.workdps(digits):
        a = lambda s: mp.mpf("0.5") + mp.mpf("0.5") / (1 + s * s)  # noqa: E731
        bb, th = (mp.mpf(10), mp.mpf(1)), (mp.mpf("0.25"), mp.mpf("0.75"))
        L = (mp.mpf(0.5), mp.mpf(-0.2)) if mode else (mp.mpf(0), mp.mpf(0))  # -0.2 the float64 the device gets
        if mode == "E":
            flux = lambda i, e: bb[i] * a(e - L[i]) * (e - L[i])  # noqa: E731
        else:
            flux = lambda i, e: bb[i] * a(e) * e + L[i]  # noqa: E731
        e2_of = lambda e1: (2 - th[0] * e1) / th[1]  # noqa: E731
        e1 = mp.findroot(lambda e: flux(0, e) - flux(1, e2_of(e)), mp.mpf("0.5"), tol=mp.mpf(10) ** (-digits + 5))
        q = flux(0, e1)
        return LD(mp.nstr(q / 2 if mode is None else q, 25))


@functools.lru_cache(maxsize=None)
def laminate_reference():
    """The unloaded laminate: (the truth at its fixed point, the mpmath value of A_H[0][0], yardsticks) with the one quantity
    ``A00`` = A_H[0][0] against mpmath: the error of secant_ref over the truth's number of rounds, relative to the value."""
    import accuracy_gpu as G
    import secant_ref as S

    base, xi, _ = laminate()
    law = soft_law("poisson", 2)
    T = iterate(geometry("p2"), law, base, xi)
    want = laminate_value(None)
    ref = S.iterate(S.solver("poisson", 2, 8), G.secant_law(law), base, xi, max_iter=T["rounds"], tol=0.0)
    e = {"A00": R.rel(ref["A"][0, 0], want)}
    return T, want, {"e": e, "bound": {k: R.bound(v, 0.0) for k, v in e.items()}}


# the groups of the GPU test: every entry is one test case of two cells (the slot cases: one)
ITERATION_CASES = [(s, fi) for s in SHAPES for fi in range(len(FAMILIES))]
RELAX = (1.0, 0.5)
TANGENT_CASES = [(s, fi) for s in SHAPES for fi in (0, 2)]  # the four kinds on both mesh classes, plain and under shear
# the scale of the macro strain of the tangent and load cases: the element tangent of psi loses definiteness where a strain entry passes 1
# (psi(s) + 2 s psi'(s) < 0 for s > 1), and the sibling plan eliminates a definite stream; the host test holds every element tangent definite
TANGENT_XI = {"mesh_ev3": 0.2, "pm3": 0.25}


def tangent_xi(shape) -> float:
    return TANGENT_XI.get(shape, 0.5)

ASYMMETRIC_CASE = ("e2", 0)
HISTORY_SHAPES = ("p2", "e2", "mesh_p2")
HISTORY_STEPS = (1.0, 1.5, 0.5)  # load, increase, unload
HISTORY_TANGENT_SHAPES = ("p2", "e2")  # potential_damage_law is written for scalar Poisson and 2D Lame
LOAD_SHAPES = ("p2", "e3", "mesh_ev3")  # one per load route: fused substitution, the blocked pass, the frontal mesh plan
STATE_CASES = {"p2": ("history", True), "e2": (None, False), "pm3": (None, None)}  # shape -> (history, eigenstrain or None for no load)
MAGNITUDE_SHAPES = ("p2", "e2", "mesh_p2")  # one per corrector route
MAGNITUDE_K = (40, -40)
SLOT_N = 112


def history_start(shape, fi=0):
    """A seeded history at the start of a state or frozen-history case: dyadic in [0, 1), so that some elements load and some do not."""
    g = geometry(shape)
    return np.random.default_rng(R.case_seed("nonlinear history", shape, fi)).integers(0, 8, (NC, g["n_el"], 1)) / 8.0


def slot_inputs():
    """The n = 112 Poisson cell of tests/test_gpu_secant.py::test_slot_path_and_lds_path_on_a_large_cell with its seeded inputs, and the
    seeded load of tests/test_gpu_secant_load.py ``_large_cell``."""
    ne = 2 * SLOT_N * SLOT_N
    rng = np.random.default_rng(12)
    d = {"coef": np.exp(rng.uniform(-1, 1, (1, ne))), "xi": rng.standard_normal((1, 2))}
    rng.integers(-8, 9, (1, 4)), rng.integers(0, 17, (ne, 2))  # the rows and points of that test: drawn to keep its load's numbers
    d["load"] = 0.3 * rng.standard_normal((1, ne, 2)) + 0.2 * rng.standard_normal((1, 1, 2))
    return d


# ------------------------------------------------------------------------------------------------------------------------------
# the references of the groups: (truth, float64 yardsticks) of one cell, computed once per process and read only
# ------------------------------------------------------------------------------------------------------------------------------

FIXED_POINT_CELLS = {"e3": 1, "mesh_ev3": 1}  # a 3D elasticity truth with its yardstick takes three seconds a cell: one cell there


def cells_of(shape) -> int:
    return FIXED_POINT_CELLS.get(shape, NC)


def _cell(shape, fi, c, xi_scale=1.0):
    coef, M, xi = inputs(shape, fi, xi_scale)
    return geometry(shape), coef[c], (None if M is None else M[c]), xi[c]


@functools.lru_cache(maxsize=None)
def iteration_reference(shape, fi, c, relax=1.0, rounds=None):
    """The softening law on cell c of (shape, family): ``rounds`` rounds, or the fixed point."""
    g, coef, M, xi = _cell(shape, fi, c)
    law = soft_law(g["kind"], g["dim"])
    T = iterate(g, law, coef, xi, M, relax=relax, rounds=rounds)
    return T, float64_errors(g, law, coef, xi, M, T, relax=relax)


@functools.lru_cache(maxsize=None)
def tangent_reference(shape, fi, c, asymmetric=False):
    """A potential law (or the asymmetric mu law) at its fixed point, and the tangent there."""
    g, coef, M, xi = _cell(shape, fi, c, tangent_xi(shape))
    law = potential_law(g["kind"], g["dim"], asymmetric)
    T = iterate(g, law, coef, xi, M)
    D = tangent(g, law, T, coef, M)
    return T, D, float64_errors(g, law, coef, xi, M, T, with_tangent=D)


@functools.lru_cache(maxsize=None)
def load_reference(shape, c, eigenstrain):
    """A potential law beside the seeded load of the cell, at its fixed point, and the tangent at the strain the law saw."""
    g, coef, M, xi = _cell(shape, 0, c, tangent_xi(shape))
    law, load = potential_law(g["kind"], g["dim"]), load_of(shape, 0)[c]
    T = iterate(g, law, coef, xi, M, load=load, eigenstrain=eigenstrain)
    D = tangent(g, law, T, coef, M)
    return T, D, float64_errors(g, law, coef, xi, M, T, load=load, eigenstrain=eigenstrain, with_tangent=D)


HISTORY_FAMILY = 1  # the top-contrast family with the mild M


@functools.lru_cache(maxsize=None)
def history_reference(shape, c):
    """The damage law along xi, 1.5 xi, 0.5 xi from a zero history, every step from the history of the step before (the truth chains its
    own, the float64 reference its own) -> [(truth, tangent, yardsticks)] of the three steps."""
    g, coef, M, xi = _cell(shape, HISTORY_FAMILY, c)
    law = damage_law(g["kind"], g["dim"])
    steps, h, h64 = [], np.zeros((g["n_el"], 1), dtype=LD), np.zeros((g["n_el"], 1))
    for scale in HISTORY_STEPS:
        T = iterate(g, law, coef, scale * xi, M, history=h)
        D = tangent(g, law, T, coef, M, history=h)
        y = float64_errors(g, law, coef, scale * xi, M, T, history=h64, with_tangent=D)
        steps.append((T, D, y))
        h, h64 = T["history"], y["history64"]
    return steps


@functools.lru_cache(maxsize=None)
def frozen_reference(shape, c):
    """``potential_damage_law`` at a seeded history (some elements load, some do not), and the tangent at that frozen history."""
    g, coef, M, xi = _cell(shape, HISTORY_FAMILY, c)
    law, h = potential_damage_law(g["kind"], g["dim"]), history_start(shape)[c]
    T = iterate(g, law, coef, xi, M, history=h)
    D = tangent(g, law, T, coef, M, history=h)
    return T, D, float64_errors(g, law, coef, xi, M, T, history=h, with_tangent=D)


STATE_THRESHOLD = {"p2": 1.0, "e2": 4.0, "pm3": 2.0}  # near the median of the truth's values


def state_case(shape):
    """(law, criterion, history[NC, ...] or None, load[NC, ...] or None, eigenstrain, labels or None) of a state case."""
    g = geometry(shape)
    hist, eig = STATE_CASES[shape]
    law = damage_law(g["kind"], g["dim"]) if hist else soft_law(g["kind"], g["dim"])
    return (law, Crit(bool(hist), STATE_THRESHOLD[shape]), history_start(shape, 1) if hist else None,
            None if eig is None else load_of(shape, 1), bool(eig), labels_of(shape) if eig is None else None)


@functools.lru_cache(maxsize=None)
def state_reference(shape, c):
    g, coef, M, xi = _cell(shape, 0, c)
    law, crit, hist, load, eig, labels = state_case(shape)
    h, P = (None if hist is None else hist[c]), (None if load is None else load[c])
    T = iterate(g, law, coef, xi, M, load=P, eigenstrain=eig, history=h)
    S = state(T, crit, coef, h, labels, 2)
    return T, S, float64_errors(g, law, coef, xi, M, T, load=P, eigenstrain=eig, history=h, with_state=S, crit=crit, labels=labels, n_regions=2)


@functools.lru_cache(maxsize=None)
def slot_reference(levels, eigenstrain):
    """Two rounds of the deep (13 levels) or the shallow (1) scalar law on the n = 112 cell, plain (None) or beside the eigenstrain."""
    g, d, law = geometry("p2", SLOT_N), slot_inputs(), deep_law(levels)
    load = d["load"][0] if eigenstrain else None
    T = iterate(g, law, d["coef"][0], d["xi"][0], load=load, eigenstrain=bool(eigenstrain), rounds=2)
    return T, float64_errors(g, law, d["coef"][0], d["xi"][0], None, T, load=load, eigenstrain=bool(eigenstrain))
