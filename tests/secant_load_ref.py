"""Test-side NumPy reference of the secant iteration beside a load (include/hommx_hip.h, hommx_secant_load_source): the
rounds of the header with ``loads_ref.Cell`` -- its own assembly, refactorised on the current stream in every round -- and
``SecantLaw.host_values``; optionally the history variables of ``history_ref`` and the tangent of ``secant_tangent_ref`` at the strain
the law saw.  One cell at a time.

Round j on the current stream c^j:  cell = Cell(c^j);  P^j = -V(c^j) E (an eigenstrain) or P;  chi_P = cell.solve(P^j);
e_K = sum_m xi_m s^m_K + eps(chi_P)_K.  A polarisation: the law reads e_K and q_K = V e_K + P_K.  An eigenstrain: it reads
g_K = e_K - E_K and q_K = V g_K.  mean_flux = sum |K| q_K; the candidate, the change and the status rules are ``secant_ref``'s.
"""

from __future__ import annotations

import numpy as np

import loads_ref as L
import secant_tangent_ref as TR


def cells(kind: str, dim: int, n: int | None = None, msh=None):
    """make(coef, M) -> ``loads_ref.Cell`` on the structured cell of n per side or on ``msh``."""
    if msh is not None:
        return lambda coef, M: L.on_mesh(msh, kind, coef, M)
    return lambda coef, M: L.structured(kind, dim, n, coef, M)


def state(make, c, M, xi, load, eigenstrain: bool) -> dict:
    """What one round sees on the stream c: ``s`` / ``q`` the strain and flux the law reads, ``e`` the total strain, ``P`` the
    polarisation of the round, ``A`` and ``mean_flux``, and the factorised ``cell``."""
    cell = make(c, M)
    load = np.asarray(load, dtype=np.float64)
    P = -np.einsum("emn,en->em", cell.V, load) if eigenstrain else load
    e = np.einsum("m,met->et", np.asarray(xi, dtype=np.float64), cell.s_canon) + cell.solve(P[None])["eps"][0]
    if eigenstrain:
        s = e - load
        q = np.einsum("emn,en->em", cell.V, s)
    else:
        s = e
        q = np.einsum("emn,en->em", cell.V, e) + P
    return {"A": cell.A, "s": s, "q": q, "e": e, "P": P, "mean_flux": np.einsum("e,et->t", cell.vol, q), "cell": cell}


def iterate(make, law, base, xi, load, eigenstrain: bool, M=None, x=None, y=None, fields=None, max_iter=50, tol=1e-10, relax=1.0,
            coef_start=None, history=None) -> dict:
    """The iteration of one cell.  base[n_el(, n_comp)], xi[t], load[n_el, t], x[3], y[n_el, d], fields[n_fields],
    history[n_el(, n_history)] for a law with history variables.  The dict of ``secant_ref.iterate`` (``history_ref.iterate``), with
    ``e``, ``P`` and ``cell`` of the stopping round."""
    base = np.asarray(base, dtype=np.float64)
    n_el = base.shape[0]
    b = base.reshape(n_el, -1)
    c = b.copy() if coef_start is None else np.array(coef_start, dtype=np.float64).reshape(n_el, -1)
    x = np.zeros(3) if x is None else np.asarray(x, dtype=np.float64)
    f = None if fields is None else np.asarray(fields, dtype=np.float64)[None]
    h_in = None if history is None else np.array(history, dtype=np.float64).reshape(n_el, law.n_history)
    kw = {} if h_in is None else {"history": h_in[None]}
    changes = []
    for j in range(max_iter):
        ref = state(make, c.reshape(base.shape), M, xi, load, eigenstrain)
        v = law.host_values(ref["s"][None], ref["q"][None], b[None], x[None], y, f, **kw)[0]
        h_out = None if h_in is None else law.host_history(ref["s"][None], ref["q"][None], b[None], x[None], y, f, **kw)[0]
        w = v if relax == 1.0 else (1.0 - relax) * c + relax * v
        with np.errstate(all="ignore"):
            top, diff = np.nanmax(np.abs(w), initial=0.0), np.nanmax(np.abs(w - c), initial=0.0)
        change = 0.0 if top == 0.0 and diff == 0.0 else diff / top
        changes.append(change)
        finite = np.isfinite(v).all() and (h_out is None or np.isfinite(h_out).all())
        status = 2 if not finite else 0 if change <= tol else 1 if j + 1 == max_iter else -1
        if status >= 0:
            break
        c = w
    if status == 2 and h_in is not None:
        h_out = h_in.copy()
    return dict(ref, coef=c.reshape(base.shape), rounds=j + 1, change=change, status=status, changes=changes, history=h_out)


def tangent(kind: str, dim: int, dlaw, r: dict, base, xi, M=None, n=None, msh=None) -> dict:
    """The consistent tangent at the state ``r`` of ``iterate``: ``T`` (symmetrised) from ``secant_tangent_ref.element_tangent`` at the
    strain the law saw, ``asymmetry`` and ``D`` = A_eff of the linear cell problem of the tangent kind with T as its coefficient."""
    T = TR.element_tangent(kind, dim, r["s"], r["coef"], base, dlaw)
    top = np.abs(T).max()
    sym = 0.5 * (T + T.transpose(0, 2, 1))
    D = cells(TR.TANGENT_KIND[kind], dim, n, msh)(TR.tangent_stream(kind, dim, sym), M).A
    return {"T": sym, "asymmetry": 0.0 if top == 0.0 else np.abs(T - T.transpose(0, 2, 1)).max() / top, "D": D}
