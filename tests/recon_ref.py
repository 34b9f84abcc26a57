"""Test-side NumPy reference of the HMM reconstruction (include/hommx_hip.h, hommx_reconstruct_batch).

Correctors come from an independent solver: ``oracle.hommx_oracle`` on the structured unit cell, ``tests/periodic_fem.solve_cell`` on any
mesh.  From them, per micro element K: s_K = xi + grad / strain of chi^xi = sum_m xi_m chi_m (shear doubled), q_K = A s_K / the stress
C : eps (Voigt order, shear not doubled), and the statistics of the library's layout.
"""

from __future__ import annotations

import numpy as np

import periodic_fem as PF
from oracle import hommx_oracle as O

PAIRS = PF.PAIRS


def _geometry(X: np.ndarray):
    """P1 gradients [e, a, d] and volumes [e] of simplices with vertices X[e, a, d]."""
    d = X.shape[2]
    Minv = np.linalg.inv(np.concatenate([np.ones(X.shape[:2] + (1,)), X], axis=2))
    J = X[:, 1:, :] - X[:, :1, :]
    return np.transpose(Minv[:, 1:, :], (0, 2, 1)), np.abs(np.linalg.det(J)) / (2.0 if d == 2 else 6.0)


def fields(kind: str, dim: int, grads, vol, el_nodes, coef, M, chi, xi) -> dict:
    """s[e, t], q[e, t] and the statistics of one cell.  chi[t, n_nodes * bs] (any gauge), xi[t]."""
    xi = np.asarray(xi, float)
    t = len(PAIRS[dim]) if kind.startswith("elasticity") else dim
    gt = np.einsum("ik,eak->eai", np.eye(dim) if M is None else np.asarray(M, float), grads)
    cx = xi @ chi  # chi^xi
    C = PF.material_tensor(kind, np.asarray(coef, float).reshape(len(vol), -1), dim)
    if kind.startswith("poisson"):
        s = xi[None, :] + np.einsum("ea,eai->ei", cx[el_nodes], gt)
        q = np.einsum("eij,ej->ei", C, s)
        nrm = np.linalg.norm(q, axis=1)
    else:
        E = PF.unit_strains(dim)
        u = cx.reshape(-1, dim)[el_nodes]  # [e, a, alpha]
        du = np.einsum("eap,eaj->epj", u, gt)  # d u_p / d y_j
        eps = np.einsum("m,mij->ij", xi, E)[None] + 0.5 * (du + np.transpose(du, (0, 2, 1)))
        sig = np.einsum("eijkl,ekl->eij", C, eps)
        s = np.stack([eps[:, k, l] * (1.0 if k == l else 2.0) for (k, l) in PAIRS[dim]], axis=1)
        q = np.stack([sig[:, k, l] for (k, l) in PAIRS[dim]], axis=1)
        nrm = np.sqrt(np.einsum("eij,eij->e", sig, sig))
    k = int(np.argmax(nrm))
    return {"s": s, "q": q, "mean_strain": vol @ s, "mean_flux": vol @ q, "energy": float(vol @ np.einsum("ei,ei->e", s, q)),
            "max_flux": float(nrm[k]), "argmax_element": k, "t": t}


def structured(kind: str, dim: int, n: int, coef, M, xi) -> dict:
    """Reference on create_unit_square / create_unit_cube(n): the oracle's cell problem, correctors and Schur-form A_H."""
    x, cells = O.unit_cell_mesh(dim, n)
    grads, vol = _geometry(x[cells])
    el_nodes = O.periodic_master_map(dim, n)[cells]
    C = PF.material_tensor(kind, np.asarray(coef, float).reshape(len(vol), -1), dim)
    okind = "poisson" if kind.startswith("poisson") else "elasticity"
    cp = O.build_cell_problem(okind, dim, n, C, M)
    chi = O.solve_correctors(cp)  # [n_dof, t]
    out = fields(kind, dim, grads, vol, el_nodes, coef, M, chi.T, xi)
    out["A"] = O.effective_tensor(cp, chi, form="schur")
    return out


def on_mesh(msh, kind: str, coef, M, xi) -> dict:
    """Reference on any periodic mesh of the unit cell (periodic_fem.solve_cell); element order of the mesh."""
    dim = msh.topology.dim
    A, chi, node = PF.solve_cell(msh, kind, coef, M)
    grads, vol = _geometry(msh.geometry.x[msh.cells][:, :, :dim])
    out = fields(kind, dim, grads, vol, node[msh.cells], coef, M, chi, xi)
    out["A"] = A
    return out


def random_coef(kind: str, dim: int, n_el: int, rng, contrast: float = 1e2) -> np.ndarray:
    """Element stream of one cell in the library's layout, log-uniform over `contrast`."""
    te = dim * (dim + 1) // 2
    g = np.exp(rng.uniform(0.0, np.log(contrast), n_el))
    if kind == "poisson":
        return g
    if kind == "poisson_matrix":
        c = np.zeros((n_el, te))
        c[:, :dim] = g[:, None] * (1.0 + 0.2 * rng.random((n_el, dim)))
        c[:, dim:] = 0.1 * g[:, None] * rng.uniform(-1, 1, (n_el, te - dim))
        return c
    if kind == "elasticity":
        return np.stack([g * rng.uniform(0.5, 1.5, n_el), g], axis=1)
    B = rng.uniform(-0.3, 0.3, (n_el, te, te))
    V = g[:, None, None] * (np.einsum("eij,ekj->eik", B, B) + np.eye(te))
    iu = np.triu_indices(te)
    return V[:, iu[0], iu[1]]


def random_M(dim: int, rng) -> np.ndarray:
    return np.eye(dim) + 0.2 * rng.uniform(-1, 1, (dim, dim))
