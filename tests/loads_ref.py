"""Test-side NumPy / SciPy reference of the cell problem with user-supplied polarisation loads (include/hommx_hip.h, hommx_loads_source;
DESIGN.md 4.10), for any periodic simplicial mesh of the unit cell and any kind, with or without M.

Its own assembly in the Voigt basis of the canonical loads: B_K maps the dofs of element K to its strain (Poisson: M grad; elasticity:
sym grad in Voigt order with the shear DOUBLED), V_K = E^m : C_K : E^n is the element operator on such strains, so that with P in Voigt
order, shear NOT doubled, strain . P is the tensor contraction:
    K = sum |K| B^T V B,    f^l = sum |K| B^T P^l,    K chi_l = -f^l   (node 0 pinned, sparse LU, returned mean-free)
    eps_l = B chi_l,  q^l = P^l + V eps_l,  P_eff[l] = sum |K| q^l,  energy[l][l'] = sum |K| eps_l . V eps_l' = -sum |K| P^l . eps_l'
    Levin: P_eff[l][m] = sum |K| (e_m + eps(chi^m)) . P^l   with chi^m the corrector of the load P = V e_m.
tests/test_loads_host.py checks it against ``periodic_fem.solve_cell`` and against its own identities before anything leans on it.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from periodic_fem import PAIRS, material_tensor, periodic_map, unit_strains
from recon_ref import random_M, random_coef  # noqa: F401  (what the tests draw their cells from)
from oracle import hommx_oracle as O


def tensor_size(kind: str, dim: int) -> int:
    return dim if kind.startswith("poisson") else len(PAIRS[dim])


def voigt_material(kind: str, coef, dim: int, n_el: int) -> np.ndarray:
    """V[e, t, t] = E^m : C_e : E^n (Poisson: A_e): material(coef) e_m is column m."""
    C = material_tensor(kind, np.asarray(coef, float).reshape(n_el, -1), dim)
    if kind.startswith("poisson"):
        return C
    E = unit_strains(dim)
    return np.einsum("mij,eijkl,nkl->emn", E, C, E)


class Cell:
    """One cell with its operator factorised once.  ``node``: vertex -> periodic node (default: ``periodic_fem.periodic_map``)."""

    def __init__(self, x, cells, kind: str, coef, M=None, node=None):
        x, cells = np.asarray(x, float), np.asarray(cells)
        dim = cells.shape[1] - 1
        self.kind, self.dim, self.t = kind, dim, tensor_size(kind, dim)
        if node is None:
            node, nn = periodic_map(x, dim)
        else:
            node = np.asarray(node)
            nn = int(node.max()) + 1
        self.nn, self.n_el = nn, len(cells)
        X = x[cells][:, :, :dim]
        self.vol = np.abs(np.linalg.det(X[:, 1:, :] - X[:, :1, :])) / (2.0 if dim == 2 else 6.0)
        Minv = np.linalg.inv(np.concatenate([np.ones(X.shape[:2] + (1,)), X], axis=2))
        gt = np.einsum("ik,eak->eai", np.eye(dim) if M is None else np.asarray(M, float), np.transpose(Minv[:, 1:, :], (0, 2, 1)))
        nv = dim + 1
        if kind.startswith("poisson"):
            self.bs = 1
            B = np.transpose(gt, (0, 2, 1))  # [e, t, a]
        else:
            self.bs = dim
            B = np.zeros((self.n_el, self.t, nv, dim))
            for m, (k, l) in enumerate(PAIRS[dim]):
                if k == l:
                    B[:, m, :, k] = gt[:, :, k]
                else:
                    B[:, m, :, k] = gt[:, :, l]
                    B[:, m, :, l] = gt[:, :, k]
            B = B.reshape(self.n_el, self.t, nv * dim)
        self.B = B
        self.rows = (node[cells][:, :, None] * self.bs + np.arange(self.bs)).reshape(self.n_el, -1)
        self.V = voigt_material(kind, coef, dim, self.n_el)
        nd, nl = nn * self.bs, self.rows.shape[1]
        self.nd = nd
        Ke = np.einsum("e,eta,etu,eub->eab", self.vol, B, self.V, B)
        K = sp.coo_matrix((Ke.ravel(), (np.repeat(self.rows, nl, axis=1).ravel(), np.tile(self.rows, (1, nl)).ravel())), shape=(nd, nd)).tocsc()
        self.keep = np.arange(self.bs, nd)
        self.lu = spla.splu(K[self.keep][:, self.keep].tocsc())
        # the canonical loads P = V e_m: their correctors, strains s^m = e_m + eps(chi^m), and A_H
        canon = self.solve(np.transpose(self.V, (2, 0, 1)))
        self.chi_canon = canon["chi"]
        self.s_canon = np.eye(self.t)[:, None, :] + canon["eps"]
        self.A = canon["P_eff"].T.copy()  # P_eff[m] = A_H[:, m]
        self.C0 = np.einsum("e,emn->mn", self.vol, self.V)

    def load_vector(self, P) -> np.ndarray:
        """f[l, nd] = sum_K |K| B_K^T P^l_K."""
        fe = np.einsum("e,eta,let->lea", self.vol, self.B, P)
        return np.stack([np.bincount(self.rows.ravel(), weights=fe[l].ravel(), minlength=self.nd) for l in range(len(P))])

    def solve(self, P) -> dict:
        """P[n_loads, n_el, t] -> chi[l, nd] (mean-free), eps / q[l, e, t], P_eff[l, t] (direct), energy / energy_P[l, l'] (both forms),
        max_flux / argmax_element[l]."""
        P = np.asarray(P, float).reshape(-1, self.n_el, self.t)
        f = self.load_vector(P)
        chi = np.zeros((len(P), self.nd))
        chi[:, self.keep] = self.lu.solve(np.ascontiguousarray(-f[:, self.keep].T)).T
        c = chi.reshape(len(P), self.nn, self.bs)
        chi = (c - c.mean(axis=1, keepdims=True)).reshape(len(P), self.nd)
        eps = np.einsum("eta,lea->let", self.B, chi[:, self.rows])
        q = P + np.einsum("etu,leu->let", self.V, eps)
        w = np.array([1.0 if (self.kind.startswith("poisson") or m < self.dim) else 2.0 for m in range(self.t)])
        nrm = np.sqrt(np.einsum("t,let->le", w, q * q))
        return {"chi": chi, "eps": eps, "q": q, "f": f, "P_eff": np.einsum("e,let->lt", self.vol, q),
                "energy": np.einsum("e,let,etu,keu->lk", self.vol, eps, self.V, eps), "energy_P": -np.einsum("e,let,ket->lk", self.vol, P, eps),
                "max_flux": nrm.max(axis=1), "argmax_element": nrm.argmax(axis=1), "norm": nrm}

    def levin(self, P) -> np.ndarray:
        """P_eff[l, m] = sum_K |K| s^m_K . P^l_K from the canonical correctors."""
        return np.einsum("e,met,let->lm", self.vol, self.s_canon, np.asarray(P, float).reshape(-1, self.n_el, self.t))


def on_mesh(msh, kind: str, coef, M=None, node=None) -> Cell:
    """On any periodic mesh of the unit cell, element order of the mesh; ``node``: the plan's ``to_periodic`` for its dof order."""
    return Cell(msh.geometry.x[:, :msh.topology.dim], msh.cells, kind, coef, M, node)


def structured(kind: str, dim: int, n: int, coef, M=None) -> Cell:
    """On create_unit_square / create_unit_cube(n) in the element and dof order of the structured plans (node = i + n j [+ n^2 k])."""
    x, cells = O.unit_cell_mesh(dim, n)
    return Cell(x, cells, kind, coef, M, O.periodic_master_map(dim, n))


def random_loads(rng, n_loads: int, n_el: int, t: int) -> np.ndarray:
    """Loads of order one with a non-zero mean: rough fields exercise every element."""
    return rng.standard_normal((n_loads, n_el, t)) + rng.standard_normal((n_loads, 1, t))


def mesh_like(x, cells):
    """A stand-in with the three attributes the references read of a mesh."""
    x = np.asarray(x, float)
    return SimpleNamespace(geometry=SimpleNamespace(x=x), cells=np.asarray(cells), topology=SimpleNamespace(dim=np.asarray(cells).shape[1] - 1))
