"""Test-side NumPy reference of the derivatives of A_H along coefficient directions (include/hommx_hip.h, hommx_sensitivity_source;
DESIGN.md 4.9), on top of the reference of the reconstruction (tests/recon_ref.py).

s^m_K: the strain of the reconstruction for xi = e_m (``recon_ref.structured`` / ``on_mesh``); material(dir) comes from
``periodic_fem.material_tensor`` and is applied as ``recon_ref.fields`` applies material(coef): q = material(dir_K) s^n_K in Voigt
order, shear not doubled, so that s^m . q^n is the energy product.  From there
    dA[d][m][n] = sum_K |K| s^m_K . material(dir_d[K]) s^n_K,      grad[K][q] = |K| sum_{m,n} w[m][n] s^m_K . material(e_q) s^n_K.
"""

from __future__ import annotations

import numpy as np

import periodic_fem as PF
import recon_ref as R
from oracle import hommx_oracle as O


def tensor_size(kind: str, dim: int) -> int:
    return dim if kind.startswith("poisson") else dim * (dim + 1) // 2


class Cell:
    """One cell problem, solved once: the strains s[m][e, t] of the t canonical loads, the element volumes, and A_H."""

    def __init__(self, kind, dim, vol, s, A):
        self.kind, self.dim, self.vol, self.s, self.A = kind, dim, vol, s, A
        self.t = len(s)

    def _q(self, dir_, n):
        """material(dir_K) s^n_K [e, t] in Voigt order, shear not doubled: the q of ``recon_ref.fields`` with `dir_` as the coefficient."""
        C = PF.material_tensor(self.kind, np.asarray(dir_, float).reshape(len(self.vol), -1), self.dim)
        s = self.s[n]
        if self.kind.startswith("poisson"):
            return np.einsum("eij,ej->ei", C, s)
        eps = np.zeros((len(self.vol), self.dim, self.dim))
        for m, (k, l) in enumerate(R.PAIRS[self.dim]):
            eps[:, k, l] = eps[:, l, k] = s[:, m] * (1.0 if k == l else 0.5)
        sig = np.einsum("eijkl,ekl->eij", C, eps)
        return np.stack([sig[:, k, l] for (k, l) in R.PAIRS[self.dim]], axis=1)

    def dA(self, dir_) -> np.ndarray:
        out = np.empty((self.t, self.t))
        for n in range(self.t):
            q = self._q(dir_, n)
            for m in range(self.t):
                out[m, n] = self.vol @ np.einsum("ei,ei->e", self.s[m], q)
        return out

    def grad(self, w, n_comp: int) -> np.ndarray:
        """[e, n_comp]: the gradient of w : A_H with respect to every coefficient entry."""
        out = np.zeros((len(self.vol), n_comp))
        for c in range(n_comp):
            unit = np.zeros((len(self.vol), n_comp))
            unit[:, c] = 1.0
            for n in range(self.t):
                q = self._q(unit, n)
                for m in range(self.t):
                    out[:, c] += w[m, n] * self.vol * np.einsum("ei,ei->e", self.s[m], q)
        return out


def structured(kind: str, dim: int, n: int, coef, M) -> Cell:
    """On create_unit_square / create_unit_cube(n): one call of ``recon_ref.structured`` per canonical load."""
    t = tensor_size(kind, dim)
    rs = [R.structured(kind, dim, n, coef, M, np.eye(t)[m]) for m in range(t)]
    x, cells = O.unit_cell_mesh(dim, n)
    return Cell(kind, dim, R._geometry(x[cells])[1], [r["s"] for r in rs], rs[0]["A"])


def on_mesh(msh, kind: str, coef, M) -> Cell:
    """On any periodic mesh of the unit cell: one call of ``recon_ref.on_mesh`` per canonical load."""
    dim = msh.topology.dim
    t = tensor_size(kind, dim)
    rs = [R.on_mesh(msh, kind, coef, M, np.eye(t)[m]) for m in range(t)]
    return Cell(kind, dim, R._geometry(msh.geometry.x[msh.cells][:, :, :dim])[1], [r["s"] for r in rs], rs[0]["A"])


def oracle_tensor(kind: str, dim: int, n: int, coef, M) -> np.ndarray:
    """A_H of the CPU oracle alone (Schur form): what the central differences differentiate."""
    C = PF.material_tensor(kind, np.asarray(coef, float).reshape((2 if dim == 2 else 6) * n**dim, -1), dim)
    cp = O.build_cell_problem("poisson" if kind.startswith("poisson") else "elasticity", dim, n, C, M)
    return O.effective_tensor(cp, O.solve_correctors(cp), form="schur")
