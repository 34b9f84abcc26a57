"""Test-side NumPy / SciPy reference of the second derivatives of A_H along coefficient directions (include/hommx_hip.h,
hommx_second_sensitivity_source), on top of the reference of the polarisation loads (tests/loads_ref.py).

With s^m = e_m + eps(chi^m) the canonical strains of ``loads_ref.Cell`` and V(c) = ``loads_ref.voigt_material`` of a stream c (linear in
c), the derivative of the canonical corrector m along dir_b is the corrector of the load P^{b,m} = V(dir_b) s^m, which ``Cell.solve``
solves; with eps_b[m] its strain
    energy form   d2A[a][b][m][n] = -sum_K |K| [ eps_b[m] . V(coef) eps_a[n] + eps_a[m] . V(coef) eps_b[n] ]         (the reference)
    direct form   g_ab[m][n] = sum_K |K| eps_b[m] . V(dir_a) s^n,  d2A[a][b] = g_ab + g_ab^T                          (what the library sums)
The two are the same number in exact arithmetic (the cell equation of chi^n_a tested with chi^m_b) and share no sum;
tests/test_sens2_host.py holds them together, and both against central second differences of the CPU oracle's A_H.
"""

from __future__ import annotations

import numpy as np

import loads_ref as L
import sens_ref as S
from loads_ref import on_mesh, random_M, random_coef, structured  # noqa: F401  (the cells the tests build)


def _operators(cell: L.Cell, dirs) -> list:
    return [L.voigt_material(cell.kind, d, cell.dim, cell.n_el) for d in dirs]


def load_strains(cell: L.Cell, dirs) -> np.ndarray:
    """eps[b][m, e, t]: the strain of d chi^m / d theta_b, the corrector of the load V(dir_b) s^m."""
    return np.stack([cell.solve(np.einsum("etu,meu->met", Vb, cell.s_canon))["eps"] for Vb in _operators(cell, dirs)])


def second_derivatives(cell: L.Cell, dirs, form: str = "energy") -> np.ndarray:
    """d2A[a, b, m, n] of ``cell`` along ``dirs[n_dirs, n_el(, n_comp)]`` by the energy form (default) or the direct form."""
    eps = load_strains(cell, dirs)
    if form == "energy":
        e = np.einsum("e,bmet,etu,aneu->abmn", cell.vol, eps, cell.V, eps)
        return -(e + np.transpose(e, (1, 0, 2, 3)))
    if form != "direct":
        raise ValueError(form)
    g = np.stack([np.einsum("e,bmet,etu,neu->bmn", cell.vol, eps, Va, cell.s_canon) for Va in _operators(cell, dirs)])
    return g + np.transpose(g, (0, 1, 3, 2))


def first_derivatives(cell: L.Cell, dirs) -> np.ndarray:
    """dA[d, m, n] = sum_K |K| s^m . V(dir_d) s^n."""
    return np.stack([np.einsum("e,met,etu,neu->mn", cell.vol, cell.s_canon, Vd, cell.s_canon) for Vd in _operators(cell, dirs)])


def central_second_differences(kind: str, dim: int, n: int, coef, M, dirs, h: float) -> np.ndarray:
    """d2A[a, b, m, n] by central second differences of the CPU oracle's A_H (``sens_ref.oracle_tensor``) with step h: three points on
    the diagonal, four off it; O(h^2) truncation, eps |A_H| / h^2 rounding."""
    coef, dirs = np.asarray(coef, float), np.asarray(dirs, float)
    A = lambda c: S.oracle_tensor(kind, dim, n, c, M)
    nd, A0 = len(dirs), A(coef)
    out = np.empty((nd, nd) + A0.shape)
    for a in range(nd):
        out[a, a] = (A(coef + h * dirs[a]) - 2.0 * A0 + A(coef - h * dirs[a])) / h**2
        for b in range(a):
            pp, pm = A(coef + h * dirs[a] + h * dirs[b]), A(coef + h * dirs[a] - h * dirs[b])
            mp, mm = A(coef - h * dirs[a] + h * dirs[b]), A(coef - h * dirs[a] - h * dirs[b])
            out[a, b] = out[b, a] = (pp - pm - mp + mm) / (4.0 * h**2)
    return out
