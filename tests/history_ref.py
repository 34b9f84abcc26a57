"""Test-side NumPy reference of the secant iteration of a law with history variables (include/hommx_hip.h, hommx_secant_history_source;
DESIGN.md 4.17): the rounds of ``secant_ref.iterate`` -- the correctors of ``recon_ref``, ``SecantLaw.host_values`` -- with the history
of the element read by every round as it was at the start of the call, and ``SecantLaw.host_history`` for the updates.  One cell at a
time.

Round j: A^j, e_K, q_K from the current stream c^j; v = law(e, q, base, x, y, f, h_in), h' = updates(e, q, base, x, y, f, h_in); the
candidate, the change and the status rules of ``secant_ref`` -- the history does not enter the change, a non-finite update counts
towards status 2 --; what comes back is the state of the stopping round with ``history`` = h' of that round, and h_in itself, bit
for bit, for status 2.
"""

from __future__ import annotations

import numpy as np

import secant_ref as S

solver = S.solver


def iterate(solve, law, base, xi, history, M=None, x=None, y=None, fields=None, max_iter=50, tol=1e-10, relax=1.0, coef_start=None) -> dict:
    """The iteration of one cell.  base[n_el(, n_comp)], xi[t], history[n_el(, n_history)], x[3], y[n_el, d], fields[n_fields]."""
    base = np.asarray(base, dtype=np.float64)
    n_el = base.shape[0]
    b = base.reshape(n_el, -1)
    h_in = np.array(history, dtype=np.float64).reshape(n_el, law.n_history)
    c = b.copy() if coef_start is None else np.array(coef_start, dtype=np.float64).reshape(n_el, -1)
    x = np.zeros(3) if x is None else np.asarray(x, dtype=np.float64)
    f = None if fields is None else np.asarray(fields, dtype=np.float64)[None]
    changes = []
    for j in range(max_iter):
        ref = solve(c.reshape(base.shape), M, xi)
        v = law.host_values(ref["s"][None], ref["q"][None], b[None], x[None], y, f, history=h_in[None])[0]
        h_out = law.host_history(ref["s"][None], ref["q"][None], b[None], x[None], y, f, history=h_in[None])[0]
        w = v if relax == 1.0 else (1.0 - relax) * c + relax * v
        with np.errstate(all="ignore"):
            top, diff = np.nanmax(np.abs(w), initial=0.0), np.nanmax(np.abs(w - c), initial=0.0)
        change = 0.0 if top == 0.0 and diff == 0.0 else diff / top
        changes.append(change)
        finite = np.isfinite(v).all() and np.isfinite(h_out).all()
        status = 2 if not finite else 0 if change <= tol else 1 if j + 1 == max_iter else -1
        if status >= 0:
            break
        c = w
    if status == 2:
        h_out = h_in.copy()
    return {"A": ref["A"], "mean_flux": ref["mean_flux"], "coef": c.reshape(base.shape), "rounds": j + 1, "change": change,
            "status": status, "changes": changes, "s": ref["s"], "q": ref["q"], "history": h_out}
