"""Test-side NumPy reference of the derivatives of A_H with respect to the stratification M (include/hommx_hip.h,
hommx_stratification_sensitivity_source), on ``loads_ref.Cell``: any periodic simplicial mesh of the unit cell, any kind.

The strain of a local dof is linear in M and C0 does not depend on it, so with the canonical correctors chi_n, their raw gradients
H^n_K[alpha][b] = sum_a chi_n[p_a bs + alpha] g_a[b] (no M), the strains s^n_K of the cell (M applied, shear doubled) and sigma^n_K = V_K s^n_K
as a d x bs matrix (Poisson: the flux vector; elasticity: the symmetric tensor, shear not doubled):
    dA_dM[a][b][m][n] = sum_K |K| [ (sigma^m_K H^n_K)[a][b] + (sigma^n_K H^m_K)[a][b] ]                      (``dA_dM``, the moment form)
Independently, with the strain operator B(M) of ``loads_ref.Cell`` and B(dM) = B(I + dM) - B(I) (B is linear in M):
    dA_H[dM][m][n] = sum_K |K| [ s^m_K . V_K B_K(dM) chi_n + B_K(dM) chi_m . V_K s^n_K ]                     (``dA_dM_operator``)
tests/test_strat_sens_host.py checks the two against each other, against central differences of the cell's own A_H and against the
exact identities before anything leans on them.
"""

from __future__ import annotations

import numpy as np

import loads_ref as L
from periodic_fem import PAIRS
from oracle import hommx_oracle as O


class StratCell:
    """``loads_ref.Cell`` of one cell with what rebuilds it for another M and the raw P1 gradients of its elements."""

    def __init__(self, x, cells, kind: str, coef, M=None, node=None):
        self.x, self.cells, self.kind, self.coef, self.node = np.asarray(x, float), np.asarray(cells), kind, np.asarray(coef, float), node
        self.cell = L.Cell(self.x, self.cells, kind, coef, M, node)
        self.dim, self.t, self.bs, self.A = self.cell.dim, self.cell.t, self.cell.bs, self.cell.A
        self.M = np.eye(self.dim) if M is None else np.asarray(M, float)
        X = self.x[self.cells][:, :, :self.dim]
        Minv = np.linalg.inv(np.concatenate([np.ones(X.shape[:2] + (1,)), X], axis=2))
        self.g = np.transpose(Minv[:, 1:, :], (0, 2, 1))  # [e, vertex, b]

    def with_M(self, M) -> "StratCell":
        return StratCell(self.x, self.cells, self.kind, self.coef, M, self.node)

    def local_correctors(self) -> np.ndarray:
        """chi[n, e, vertex, alpha] of the canonical correctors."""
        c = self.cell
        return c.chi_canon[:, c.rows].reshape(c.t, c.n_el, self.dim + 1, c.bs)

    def stress_matrices(self) -> np.ndarray:
        """sigma[m, e, a, alpha] of the canonical loads."""
        c = self.cell
        sv = np.einsum("etu,meu->met", c.V, c.s_canon)
        if self.kind.startswith("poisson"):
            return sv[..., None]
        sig = np.zeros((c.t, c.n_el, self.dim, self.dim))
        for q, (k, l) in enumerate(PAIRS[self.dim]):
            sig[:, :, k, l] = sig[:, :, l, k] = sv[:, :, q]
        return sig


def dA_dM(sc: StratCell) -> np.ndarray:
    """[d, d, t, t] by the moment form."""
    H = np.einsum("nevx,evb->nexb", sc.local_correctors(), sc.g)  # [n, e, alpha, b]
    half = np.einsum("e,meax,nexb->abmn", sc.cell.vol, sc.stress_matrices(), H)
    return half + np.swapaxes(half, 2, 3)


def dA_dM_operator(sc: StratCell) -> np.ndarray:
    """[d, d, t, t] by the strain operator built with dM = E_ab in place of M."""
    c, d = sc.cell, sc.dim
    B0 = sc.with_M(np.eye(d)).cell.B
    chi = c.chi_canon[:, c.rows]  # [n, e, local dof]
    out = np.empty((d, d, c.t, c.t))
    for a in range(d):
        for b in range(d):
            E = np.zeros((d, d))
            E[a, b] = 1.0
            dB = sc.with_M(np.eye(d) + E).cell.B - B0
            half = np.einsum("e,met,etu,eux,nex->mn", c.vol, c.s_canon, c.V, dB, chi)
            out[a, b] = half + half.T
    return out


def grad_M(sc: StratCell, w) -> np.ndarray:
    """[d, d] = sum_mn w[m][n] dA_dM[a][b][m][n], formed as the kernel forms it: sum_K |K| sum_n (V^n H^n)[a][b] with
    V^n = sum_m (w[m][n] + w[n][m]) sigma^m -- no t x t intermediate."""
    w = np.asarray(w, float)
    H = np.einsum("nevx,evb->nexb", sc.local_correctors(), sc.g)
    V = np.einsum("mn,meax->neax", w + w.T, sc.stress_matrices())
    return np.einsum("e,neax,nexb->ab", sc.cell.vol, V, H)


def central_difference(sc: StratCell, h: float = 1e-6) -> np.ndarray:
    """[d, d, t, t]: central differences of the cell's own A_H along every unit direction E_ab."""
    d = sc.dim
    out = np.empty((d, d, sc.t, sc.t))
    for a in range(d):
        for b in range(d):
            E = np.zeros((d, d))
            E[a, b] = h
            out[a, b] = (sc.with_M(sc.M + E).A - sc.with_M(sc.M - E).A) / (2 * h)
    return out


def on_mesh(msh, kind: str, coef, M=None, node=None) -> StratCell:
    """On any periodic mesh of the unit cell, element order of the mesh; ``node``: the plan's ``to_periodic`` for its dof order."""
    return StratCell(msh.geometry.x[:, :msh.topology.dim], msh.cells, kind, coef, M, node)


def structured(kind: str, dim: int, n: int, coef, M=None) -> StratCell:
    """On create_unit_square / create_unit_cube(n) in the element and dof order of the structured plans."""
    x, cells = O.unit_cell_mesh(dim, n)
    return StratCell(x, cells, kind, coef, M, O.periodic_master_map(dim, n))


def laminate_coef(n: int, a) -> np.ndarray:
    """Element stream of the structured 2D Poisson cell whose coefficient a[i] depends on the element column alone (element 2 (i + n j) + s)."""
    return np.repeat(np.tile(np.asarray(a, float), n), 2)


def laminate_exact(a, M) -> tuple[np.ndarray, np.ndarray]:
    """(A_H[2, 2], dA_dM[2, 2, 2, 2]) of that cell, where the P1 corrector is exact: with v = M[:, 0],
    A_H = <a> I - (<a> - a_harm) v v^T / |v|^2, which depends on the first column of M alone."""
    a, M = np.asarray(a, float), np.asarray(M, float)
    mean, harm = a.mean(), 1.0 / (1.0 / a).mean()
    v = M[:, 0]
    vv = v @ v
    A = mean * np.eye(2) - (mean - harm) * np.outer(v, v) / vv
    dA = np.zeros((2, 2, 2, 2))
    for k in range(2):
        dv = np.eye(2)[k]
        dA[k, 0] = -(mean - harm) * ((np.outer(dv, v) + np.outer(v, dv)) / vv - 2.0 * (v @ dv) * np.outer(v, v) / vv**2)
    return A, dA
