"""Test-side reference for cell problems on ANY periodic simplicial mesh of the unit cell (SciPy, float64).

Independent of the package: its own periodic matching (rounded coordinates), its own element matrices (the full Hooke tensor /
the matrix A contracted with the P1 gradients, as in the literal forms of hmm.py:644-667 / 887-922 and their stratified versions),
its own gauge (node 0 pinned, sparse LU).  Pinned against ``oracle.hommx_oracle`` on structured meshes in tests/test_mesh_host.py
before it checks the mesh route on unstructured ones.
"""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

PAIRS = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]}


def periodic_map(x: np.ndarray, dim: int) -> tuple[np.ndarray, int]:
    """vertex -> periodic node (nodes numbered in order of first appearance of their folded coordinate), and the node count."""
    y = np.mod(np.round(x[:, :dim] * 1e8), 1e8).astype(np.int64)
    _, first, inv = np.unique(y, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.ravel()], len(first)


def unit_strains(dim: int) -> np.ndarray:
    E = np.zeros((len(PAIRS[dim]), dim, dim))
    for m, (k, l) in enumerate(PAIRS[dim]):
        E[m, k, l] += 0.5
        E[m, l, k] += 0.5
    return E


def material_tensor(kind: str, coef: np.ndarray, dim: int) -> np.ndarray:
    """Per element: A[e, d, d] (Poisson kinds) or the Hooke tensor C[e, d, d, d, d] (elasticity kinds)."""
    coef = np.asarray(coef, dtype=float)
    ne = coef.shape[0]
    if kind == "poisson":
        return coef.reshape(ne)[:, None, None] * np.eye(dim)
    if kind == "poisson_matrix":
        A = np.zeros((ne, dim, dim))
        for m, (k, l) in enumerate(PAIRS[dim]):
            A[:, k, l] = A[:, l, k] = coef[:, m]
        return A
    I = np.eye(dim)
    if kind == "elasticity":
        lam, mu = coef[:, 0], coef[:, 1]
        return (lam[:, None, None, None, None] * np.einsum("ij,kl->ijkl", I, I)
                + mu[:, None, None, None, None] * (np.einsum("ik,jl->ijkl", I, I) + np.einsum("il,jk->ijkl", I, I)))
    # Voigt: coef holds the upper triangle of V[m, n] = E^m : C : E^n; C = sum V[m, n] F^m (x) F^n with F^m the dual basis of E^m
    t = len(PAIRS[dim])
    V = np.zeros((ne, t, t))
    iu = np.triu_indices(t)
    V[:, iu[0], iu[1]] = coef
    V[:, iu[1], iu[0]] = coef
    F = np.zeros((t, dim, dim))
    for m, (k, l) in enumerate(PAIRS[dim]):
        if k == l:
            F[m, k, k] = 1.0
        else:
            F[m, k, l] = F[m, l, k] = 1.0  # F^m : E^n = delta_mn
    return np.einsum("emn,mij,nkl->eijkl", V, F, F)


def solve_cell(msh, kind: str, coef: np.ndarray, M: np.ndarray | None = None):
    """(A_H[t, t], correctors[t, n_nodes * bs] mean-free, vertex -> node map) of one cell problem on ``msh``."""
    dim = msh.topology.dim
    x = msh.geometry.x
    cells = np.asarray(msh.cells)
    node, nn = periodic_map(x, dim)
    X = x[cells][:, :, :dim]
    J = X[:, 1:, :] - X[:, :1, :]
    vol = np.abs(np.linalg.det(J)) / (2.0 if dim == 2 else 6.0)
    Minv = np.linalg.inv(np.concatenate([np.ones(X.shape[:2] + (1,)), X], axis=2))
    g = np.transpose(Minv[:, 1:, :], (0, 2, 1))  # [e, a, dim]
    gt = np.einsum("ik,eak->eai", np.eye(dim) if M is None else np.asarray(M, float), g)
    C = material_tensor(kind, coef, dim)
    ne, nv = cells.shape
    if kind.startswith("poisson"):
        bs = 1
        Ke = np.einsum("e,eai,eij,ebj->eab", vol, gt, C, gt)
        Be = -np.einsum("e,eai,eim->eam", vol, gt, C)
        C0 = np.einsum("e,eij->ij", vol, C)
        rows = node[cells]
    else:
        bs = dim
        I = np.eye(dim)
        E = unit_strains(dim)
        eps = 0.5 * (np.einsum("pi,eaj->eapij", I, gt) + np.einsum("pj,eai->eapij", I, gt))
        Ke = np.einsum("e,eapij,eijkl,ebqkl->eapbq", vol, eps, C, eps).reshape(ne, nv * bs, nv * bs)
        Be = -np.einsum("e,eapij,eijkl,mkl->eapm", vol, eps, C, E).reshape(ne, nv * bs, -1)
        C0 = np.einsum("e,mij,eijkl,nkl->mn", vol, E, C, E)
        rows = (node[cells][:, :, None] * bs + np.arange(bs)).reshape(ne, -1)
    nd = nn * bs
    nl = rows.shape[1]
    K = sp.coo_matrix((Ke.ravel(), (np.repeat(rows, nl, axis=1).ravel(), np.tile(rows, (1, nl)).ravel())), shape=(nd, nd)).tocsc()
    t = Be.shape[2]
    B = np.stack([np.bincount(rows.ravel(), weights=Be[:, :, m].ravel(), minlength=nd) for m in range(t)], axis=1)
    keep = np.arange(bs, nd)
    chi = np.zeros((nd, t))
    chi[keep] = spla.splu(K[keep][:, keep].tocsc()).solve(np.ascontiguousarray(B[keep]))
    AH = C0 - B.T @ chi
    chi = chi.reshape(nn, bs, t)
    chi -= chi.mean(axis=0, keepdims=True)
    return AH, chi.reshape(nd, t).T.copy(), node
