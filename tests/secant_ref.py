"""Test-side NumPy reference of the secant iteration of a strain-dependent coefficient (include/hommx_hip.h, hommx_secant_source;
DESIGN.md 4.15): the same rounds with the correctors of ``recon_ref.structured`` / ``recon_ref.on_mesh`` and ``SecantLaw.host_values``,
and the status rules of the header.  One cell at a time.

Round j: A^j, e_K, q_K from the current stream c^j by the independent solver; v = law(e, q, base, x, y, f); w = v (relax == 1) or
(1 - relax) c^j + relax v; change = max |w - c^j| / max |w| (0 when both are 0); stop with 2 (v not finite), 0 (change <= tol) or 1
(j + 1 == max_iter), else c^{j+1} = w.  What comes back is the state of the stopping round: ``A``, ``mean_flux``, ``coef`` = c^j,
``rounds`` = j + 1, ``change``, ``status``, and ``changes``, the change of every round.  Status 3 (a flagged pivot) belongs to the
elimination of the library and has no counterpart here.
"""

from __future__ import annotations

import numpy as np

import recon_ref as R


def solver(kind: str, dim: int, n: int | None = None, msh=None):
    """solve(coef, M, xi) -> the dict of recon_ref for one cell, on the structured cell of n per side or on `msh`."""
    if msh is not None:
        return lambda coef, M, xi: R.on_mesh(msh, kind, coef, M, xi)
    return lambda coef, M, xi: R.structured(kind, dim, n, coef, M, xi)


def iterate(solve, law, base, xi, M=None, x=None, y=None, fields=None, max_iter=50, tol=1e-10, relax=1.0, coef_start=None) -> dict:
    """The iteration of one cell.  base[n_el(, n_comp)], xi[t], x[3], y[n_el, d], fields[n_fields]."""
    base = np.asarray(base, dtype=np.float64)
    n_el = base.shape[0]
    b = base.reshape(n_el, -1)
    c = b.copy() if coef_start is None else np.array(coef_start, dtype=np.float64).reshape(n_el, -1)
    x = np.zeros(3) if x is None else np.asarray(x, dtype=np.float64)
    f = None if fields is None else np.asarray(fields, dtype=np.float64)[None]
    changes = []
    for j in range(max_iter):
        ref = solve(c.reshape(base.shape), M, xi)
        v = law.host_values(ref["s"][None], ref["q"][None], b[None], x[None], y, f)[0]
        w = v if relax == 1.0 else (1.0 - relax) * c + relax * v
        with np.errstate(all="ignore"):
            top, diff = np.nanmax(np.abs(w), initial=0.0), np.nanmax(np.abs(w - c), initial=0.0)
        change = 0.0 if top == 0.0 and diff == 0.0 else diff / top
        changes.append(change)
        status = 2 if not np.isfinite(v).all() else 0 if change <= tol else 1 if j + 1 == max_iter else -1
        if status >= 0:
            break
        c = w
    return {"A": ref["A"], "mean_flux": ref["mean_flux"], "coef": c.reshape(base.shape), "rounds": j + 1, "change": change,
            "status": status, "changes": changes, "s": ref["s"], "q": ref["q"]}
