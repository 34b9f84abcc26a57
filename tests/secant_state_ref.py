"""Test-side NumPy reference of a criterion on the nonlinear state (include/hommx_hip.h, hommx_secant_state_source): the
rounds of ``secant_load_ref.iterate`` -- without a load the same rounds beside a zero polarisation, whose corrector is zero: the rounds
of ``history_ref`` / ``secant_ref`` --, then the criterion's total strain and flux on the stopping round's stream (``state()`` of
secant_load_ref returns ``e``, ``P`` and the factorised cell), then ``Criterion.host_values(..., base=, history=)`` and the statistics
by the rules of the header: a NaN never wins the maximum, the smallest element reaches it, the threshold counts volume.  One cell at a
time.
"""

from __future__ import annotations

import numpy as np

import secant_load_ref as SL


def statistics(v: np.ndarray, vol: np.ndarray, threshold: float) -> dict:
    """max / argmax / mean / exceed_volume of the values v[n_el] of one cell with the element volumes vol[n_el]."""
    best, arg = -np.inf, -1
    for k, x in enumerate(v):  # a NaN is greater than nothing; the first element to reach the maximum keeps it
        if x > best:
            best, arg = x, k
    return {"max": best, "argmax_element": arg, "mean": float((vol * v).sum()), "exceed_volume": float(vol[v >= threshold].sum())}


def evaluate(make, law, crit, base, xi, load=None, eigenstrain: bool = False, M=None, x=None, y=None, fields=None, crit_fields=None,
             history=None, **limits) -> dict:
    """The iteration of one cell (the dict of ``secant_load_ref.iterate``) and, on the state it stops in, ``total_strain``,
    ``total_flux``, ``values`` and the statistics of ``crit``.  base[n_el(, n_comp)], xi[t], load[n_el, t] or None, x[3], y[n_el, d],
    fields / crit_fields: the law's and the criterion's own, history[n_el(, n_history)] for a law with history variables; ``limits``:
    max_iter, tol, relax."""
    base = np.asarray(base, dtype=np.float64)
    n_el = base.shape[0]
    x = np.zeros(3) if x is None else np.asarray(x, dtype=np.float64)
    t = len(np.atleast_1d(xi))
    P = np.zeros((n_el, t)) if load is None else np.asarray(load, dtype=np.float64)
    r = SL.iterate(make, law, base, xi, P, bool(eigenstrain) and load is not None, M, x, y, fields, history=history, **limits)
    cell = r["cell"]
    e = r["e"]  # the total strain, beside an eigenstrain too
    q = np.einsum("emn,en->em", cell.V, e) + r["P"]  # material(c^j) e + P, P the polarisation or the eigenstress of the round
    kw = {}
    if history is not None:
        kw["history"] = np.asarray(history, dtype=np.float64).reshape(1, n_el, -1)
    f = None if crit_fields is None else np.asarray(crit_fields, dtype=np.float64)[None]
    v = crit.host_values(e[None], q[None], r["coef"][None], x[None], y, f, base=base[None], **kw)[0]
    return dict(r, total_strain=e, total_flux=q, values=v, **statistics(v, cell.vol, crit.threshold))
