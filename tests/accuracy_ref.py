"""Extended-precision reference for the cell problems (NumPy ``longdouble``, eps 1.1e-19; no GPU), and the float64 yardsticks.

``truth`` assembles the periodic P1 cell problem of ANY periodic simplicial mesh in long double -- element gradients (adjugate
formulas: no LAPACK, which has no long double), volumes, element matrices, loads and C0, all from the float64 inputs -- solves it, and
evaluates the effective tensor in the energy form  sum_e vol (E^m + eps(chi_m)) : C : (E^n + eps(chi_n)),  which has no cancellation.
Two solvers: a dense long-double Cholesky of the pinned system (N <~ 400), and float64 sparse LU refined with long-double residuals
until the correction is below 1e-17 relative (any size).  tests/test_accuracy_ref_host.py holds the two against each other, against a
40-digit mpmath solve, and the structured against the mesh path.

``float64_errors`` measures, against that truth, what float64 delivers on the same inputs with (i) the oracle's Schur form
C0 - B^T K^-1 B (oracle/hommx_oracle.py on structured cells, tests/periodic_fem.py on meshes) and (ii) a dense Cholesky evaluation of
the same form.  The HIP kernels evaluate this form too, so these two errors are the yardstick of tests/test_gpu_accuracy.py:

    e_gpu <= FACTOR * max(e_oracle_schur, e_cholesky_schur, FLOOR_EPS * eps),      FACTOR = 32, FLOOR_EPS = 16.

The case tables and coefficient families of the GPU accuracy tests live here too, so that the host test can hold the yardstick itself
below 1e-12 on every family (an ill-posed input cannot loosen a bound unnoticed) and tools/accuracy_table.py can reuse them.

``derived_truth`` extends the truth to everything the package computes FROM the correctors (reconstruction, coefficient and stratification
derivatives, load responses, second coefficient derivatives); ``derived_float64_errors`` measures the float64 NumPy references of the coarse tests against it, per
quantity: the yardsticks of tests/test_gpu_accuracy_derived.py.  ``stratification_family`` holds the M families (mild, shear30,
squeeze16, rot) of the stratification tests.
"""

from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FACTOR = 32.0
FLOOR_EPS = 16.0
STALL_LIMIT = 1e-15  # largest stalled correction accepted: two orders below the smallest bound a test applies (32 * 16 eps = 1.1e-13)
PAIRS = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]}
KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")


def bound(e_oracle: float, e_cholesky: float) -> float:
    """The bound of the GPU accuracy tests from the two float64 yardstick errors (never from a GPU result)."""
    return FACTOR * max(e_oracle, e_cholesky, FLOOR_EPS * EPS)


# ------------------------------------------------------------------------------------------------------------------------------
# assembly, generic in the number format (long double for the truth, float64 for the Cholesky yardstick)
# ------------------------------------------------------------------------------------------------------------------------------


def unit_strains(dim: int, dtype=LD) -> np.ndarray:
    E = np.zeros((len(PAIRS[dim]), dim, dim), dtype=dtype)
    for m, (k, l) in enumerate(PAIRS[dim]):
        E[m, k, l] += dtype(0.5)
        E[m, l, k] += dtype(0.5)
    return E


def material_tensor(kind: str, coef: np.ndarray, dim: int, dtype=LD) -> np.ndarray:
    """A[e, d, d] (Poisson kinds) or C[e, d, d, d, d] (elasticity kinds) in ``dtype`` from the float64 coefficient stream of the C ABI.
    A stream that is long double already keeps its digits: the iterates of tests/nonlinear_truth.py, which float64 cannot hold."""
    coef = np.asarray(coef)
    coef = coef.astype(dtype) if coef.dtype == LD else coef.astype(np.float64).astype(dtype)
    ne = coef.shape[0]
    I = np.eye(dim, dtype=dtype)
    if kind == "poisson":
        return coef.reshape(ne)[:, None, None] * I
    if kind == "poisson_matrix":
        A = np.zeros((ne, dim, dim), dtype=dtype)
        for m, (k, l) in enumerate(PAIRS[dim]):
            A[:, k, l] = A[:, l, k] = coef[:, m]
        return A
    if kind == "elasticity":
        lam, mu = coef[:, 0], coef[:, 1]
        return (lam[:, None, None, None, None] * np.einsum("ij,kl->ijkl", I, I)
                + mu[:, None, None, None, None] * (np.einsum("ik,jl->ijkl", I, I) + np.einsum("il,jk->ijkl", I, I)))
    if kind != "elasticity_voigt":
        raise ValueError(kind)
    t = len(PAIRS[dim])
    V = np.zeros((ne, t, t), dtype=dtype)
    iu = np.triu_indices(t)
    V[:, iu[0], iu[1]] = coef
    V[:, iu[1], iu[0]] = coef
    F = np.zeros((t, dim, dim), dtype=dtype)  # dual basis of the unit strains: F^m : E^n = delta_mn
    for m, (k, l) in enumerate(PAIRS[dim]):
        F[m, k, l] = F[m, l, k] = 1
    return np.einsum("emn,mij,nkl->eijkl", V, F, F)


def element_geometry(x: np.ndarray, cells: np.ndarray, dim: int, dtype=LD):
    """P1 gradients[e, a, d] and volumes[e] by the adjugate of the edge matrix, in ``dtype``."""
    X = np.asarray(x, dtype=np.float64)[np.asarray(cells)][:, :, :dim].astype(dtype)
    J = X[:, 1:, :] - X[:, :1, :]  # rows: edges x_a - x_0
    if dim == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        inv = np.empty_like(J)  # inv[e, i, a] = (J^-1)[i][a]
        inv[:, 0, 0], inv[:, 0, 1] = J[:, 1, 1], -J[:, 0, 1]
        inv[:, 1, 0], inv[:, 1, 1] = -J[:, 1, 0], J[:, 0, 0]
        fact = 2
    else:
        r0, r1, r2 = J[:, 0], J[:, 1], J[:, 2]
        c0, c1, c2 = np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)
        det = np.einsum("ei,ei->e", r0, c0)
        inv = np.stack([c0, c1, c2], axis=2)
        fact = 6
    inv = inv / det[:, None, None]
    g = np.empty(X.shape, dtype=dtype)
    g[:, 1:, :] = np.transpose(inv, (0, 2, 1))  # grad lambda_a = column a of J^-1
    g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
    return g, np.abs(det) / dtype(fact)


class Assembled:
    """Element-level form of one cell problem in one number format."""

    def __init__(self, kind, x, cells, to_periodic, coef, M, dtype):
        cells = np.asarray(cells)
        dim = cells.shape[1] - 1
        g, vol = element_geometry(x, cells, dim, dtype)
        Mm = np.eye(dim, dtype=dtype) if M is None else np.asarray(M, dtype=np.float64).astype(dtype)
        gt = np.einsum("ik,eak->eai", Mm, g)
        C = material_tensor(kind, coef, dim, dtype)
        node = np.asarray(to_periodic)[cells]
        ne, nv = cells.shape
        self.dim, self.dtype, self.vol, self.C = dim, dtype, vol, C
        self.nn = int(np.asarray(to_periodic).max()) + 1
        if kind.startswith("poisson"):
            self.bs = 1
            self.xi = gt
            self.Ke = np.einsum("e,eai,eij,ebj->eab", vol, gt, C, gt)
            self.Be = -np.einsum("e,eai,eim->eam", vol, gt, C)
            self.C0 = np.einsum("e,eij->ij", vol, C)
            self.rows = node
        else:
            self.bs = dim
            I = np.eye(dim, dtype=dtype)
            self.E = unit_strains(dim, dtype)
            half = dtype(0.5)
            eps = half * (np.einsum("pi,eaj->eapij", I, gt) + np.einsum("pj,eai->eapij", I, gt))
            self.xi = eps
            Ceps = np.einsum("eijkl,ebqkl->ebqij", C, eps)
            self.Ke = np.einsum("e,eapij,ebqij->eapbq", vol, eps, Ceps).reshape(ne, nv * dim, nv * dim)
            self.Be = -np.einsum("e,eapij,mij->eapm", vol, Ceps, self.E).reshape(ne, nv * dim, -1)
            self.C0 = np.einsum("e,mij,eijkl,nkl->mn", vol, self.E, C, self.E)
            self.rows = (node[:, :, None] * dim + np.arange(dim)).reshape(ne, -1)
        self.t = self.Be.shape[2]
        self.nd = self.nn * self.bs

    def load(self) -> np.ndarray:
        B = np.zeros((self.nd, self.t), dtype=self.dtype)
        np.add.at(B, self.rows.ravel(), self.Be.reshape(-1, self.t))
        return B

    def matvec(self, X: np.ndarray) -> np.ndarray:
        Y = np.zeros_like(X)
        np.add.at(Y, self.rows.ravel(), np.einsum("eab,ebt->eat", self.Ke, X[self.rows]).reshape(-1, X.shape[1]))
        return Y

    def dense(self) -> np.ndarray:
        K = np.zeros((self.nd, self.nd), dtype=self.dtype)
        nl = self.rows.shape[1]
        np.add.at(K, (np.repeat(self.rows, nl, axis=1).ravel(), np.tile(self.rows, (1, nl)).ravel()), self.Ke.ravel())
        return K

    def sparse64(self) -> sp.csc_matrix:
        nl = self.rows.shape[1]
        r, c = np.repeat(self.rows, nl, axis=1).ravel(), np.tile(self.rows, (1, nl)).ravel()
        return sp.coo_matrix((self.Ke.astype(np.float64).ravel(), (r, c)), shape=(self.nd, self.nd)).tocsc()

    def energy(self, chi: np.ndarray) -> np.ndarray:
        """sum_e vol (E^m + eps(chi_m)) : C : (E^n + eps(chi_n)) -- the literal functional, no cancellation."""
        ce = chi[self.rows]  # [e, local dof, t]
        if self.bs == 1:
            F = np.einsum("eam,eai->emi", ce, self.xi) + np.eye(self.dim, dtype=self.dtype)[None]
            return np.einsum("e,emi,eij,enj->mn", self.vol, F, self.C, F)
        ne = ce.shape[0]
        F = np.einsum("eapm,eapij->emij", ce.reshape(ne, -1, self.dim, self.t), self.xi) + self.E[None]
        return np.einsum("e,emij,eijkl,enkl->mn", self.vol, F, self.C, F)

    def mean_free(self, chi: np.ndarray) -> np.ndarray:
        c = chi.reshape(self.nn, self.bs, -1)
        return (c - c.mean(axis=0, keepdims=True)).reshape(self.nd, -1)


def _cholesky_solve_ld(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """Dense Cholesky solve in the number format of A (right-looking, vectorised rows; O(N^3) long-double operations)."""
    A = A.copy()
    N = A.shape[0]
    L = np.zeros_like(A)
    for k in range(N):
        d = np.sqrt(A[k, k])
        L[k, k] = d
        col = A[k + 1:, k] / d
        L[k + 1:, k] = col
        A[k + 1:, k + 1:] -= np.outer(col, col)
    Y = B.copy()
    for k in range(N):
        Y[k] /= L[k, k]
        Y[k + 1:] -= np.outer(L[k + 1:, k], Y[k])
    for k in range(N - 1, -1, -1):
        Y[k] /= L[k, k]
        Y[:k] -= np.outer(L[k, :k], Y[k])
    return Y


def solve_ld(a: "Assembled", B: np.ndarray, solver: str = "refine") -> np.ndarray:
    """K chi = B in long double for any right-hand side B[n_dof, r] orthogonal to the constants; the dofs of node 0 pinned to zero.

    solver='dense': long-double Cholesky of the pinned system (N <~ 400).
    solver='refine': float64 sparse LU of the same system, refined with long-double residuals until the correction is below 1e-17 of
    the solution (max norm)."""
    chi = np.zeros_like(B)
    keep = np.arange(a.bs, a.nd)
    if solver == "dense":
        K = a.dense()
        chi[keep] = _cholesky_solve_ld(K[np.ix_(keep, keep)], B[keep])
    elif solver == "refine":
        K64 = a.sparse64()
        lu = spla.splu(K64[keep][:, keep].tocsc())
        prev = np.inf
        for it in range(40):
            r = (B - a.matvec(chi))[keep]
            scale = np.abs(r).max(axis=0)  # keep the float64 solve in range whatever the magnitude of the coefficient
            scale[scale == 0] = 1
            dx = lu.solve(np.ascontiguousarray((r / scale).astype(np.float64))).astype(LD) * scale
            chi[keep] += dx
            step = float(np.abs(dx).max() / np.abs(chi).max())
            if step <= 1e-17:
                break
            # the long-double residual carries noise eps_ld |K| |chi|, so on a badly conditioned cell the correction stalls at about
            # cond(K) eps_ld before it reaches 1e-17, wandering a little from step to step (hence not before the sixth).  Long double itself carries K only to eps_ld, so this is the accuracy of
            # the truth's correctors (worst case of the tests: 2D elasticity n = 25 at 1e5, second cell, 2e-16 .. 8e-16; all others reach
            # 1e-17); the energy form is second order in it.  A stall above STALL_LIMIT could decide a test: an error.
            if it >= 5 and step >= 0.25 * prev:
                if step > STALL_LIMIT:
                    raise RuntimeError(f"iterative refinement stalled at {step:.1e}: the cell problem is ill-posed")
                break
            prev = step
        else:
            raise RuntimeError("iterative refinement did not converge: the cell problem is ill-posed")
    else:
        raise ValueError(solver)
    return chi


def truth(kind, x, cells, to_periodic, coef, M=None, solver: str = "refine"):
    """(A_H[t, t], mean-free correctors[n_dof, t]) in long double; dof = periodic node * bs + component (solvers: ``solve_ld``)."""
    a = Assembled(kind, x, cells, to_periodic, coef, M, LD)
    chi = solve_ld(a, a.load(), solver)
    return a.energy(chi), a.mean_free(chi)


# ------------------------------------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------------------------------------


def structured(dim: int, n: int):
    """(x, cells, to_periodic) of the structured unit cell, from the oracle."""
    from oracle import hommx_oracle as O

    x, cells = O.unit_cell_mesh(dim, n)
    return x, cells, O.periodic_master_map(dim, n)


def mesh_arrays(msh):
    """(x, cells, to_periodic) of a package mesh with the periodic nodes the mesh plans use."""
    from hommx_amd import fem
    from hommx_amd.cell_problem import create_periodic_boundary_conditions

    mpc = create_periodic_boundary_conditions(fem.FunctionSpace(msh, 1))
    return msh.geometry.x[:, : msh.topology.dim], np.asarray(msh.cells), np.asarray(mpc.to_periodic, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 yardsticks
# ------------------------------------------------------------------------------------------------------------------------------


def rel(A, T) -> float:
    T = np.asarray(T, dtype=LD)
    return float(np.abs(np.asarray(A, dtype=LD) - T).max() / np.abs(T).max())


def _oracle_inputs(kind, coef, dim):
    """The oracle's kinds take the scalar / (lambda, mu) stream as it is and full tensors otherwise."""
    if kind in ("poisson", "elasticity"):
        return kind, np.asarray(coef, dtype=np.float64)
    return ("poisson" if kind == "poisson_matrix" else "elasticity"), material_tensor(kind, coef, dim, np.float64)


def float64_errors(kind, x, cells, to_periodic, coef, M=None, T=None, n: int | None = None, msh=None) -> dict:
    """Errors against ``truth`` (T = its result, computed here when None) of float64 on the same inputs:

    e_oracle    the oracle's Schur form: oracle.hommx_oracle on the structured cell with ``n`` cells per side, tests/periodic_fem.py on ``msh``
    e_cholesky  dense Cholesky of the pinned float64 matrix, A_H = C0 - (L^-1 B)^T (L^-1 B)
    e_corr      the oracle's (periodic_fem's) mean-free correctors
    plus ``bound`` / ``bound_corr``, the bounds the GPU tests use."""
    from oracle import hommx_oracle as O

    if T is None:
        T = truth(kind, x, cells, to_periodic, coef, M)
    AT, chiT = T
    dim = np.asarray(cells).shape[1] - 1
    if msh is None:
        okind, ocoef = _oracle_inputs(kind, coef, dim)
        cp = O.build_cell_problem(okind, dim, n, ocoef, M)
        chi = O.solve_correctors(cp)
        A_or = O.effective_tensor(cp, chi, form="schur")
        chi = chi.reshape(cp.K.shape[0] // cp.bs, cp.bs, -1)
        chi = (chi - chi.mean(axis=0, keepdims=True)).reshape(cp.K.shape[0], -1)
    else:
        import periodic_fem as PF

        A_or, chi_t, node = PF.solve_cell(msh, kind, coef, M)
        # periodic_fem numbers the periodic nodes itself: carry its correctors over to ``to_periodic`` through the mesh vertices
        bs = chi_t.shape[1] // (int(node.max()) + 1)
        nn = int(np.asarray(to_periodic).max()) + 1
        chi = np.zeros((nn, bs, chi_t.shape[0]))
        chi[np.asarray(to_periodic)] = chi_t.T.reshape(-1, bs, chi_t.shape[0])[node]
        chi = chi.reshape(nn * bs, -1)
    a = Assembled(kind, x, cells, to_periodic, coef, M, np.float64)
    keep = np.arange(a.bs, a.nd)
    L = sla.cholesky(a.dense()[np.ix_(keep, keep)], lower=True)
    Y = sla.solve_triangular(L, a.load()[keep], lower=True)
    A_ch = a.C0 - Y.T @ Y
    e_or, e_ch, e_corr = rel(A_or, AT), rel(A_ch, AT), rel(chi, chiT)
    return {"e_oracle": e_or, "e_cholesky": e_ch, "e_corr": e_corr, "bound": bound(e_or, e_ch), "bound_corr": bound(e_corr, 0.0)}


# ------------------------------------------------------------------------------------------------------------------------------
# derived outputs: reconstruction, coefficient and stratification derivatives, load responses
# ------------------------------------------------------------------------------------------------------------------------------


def tensor_size(kind: str, dim: int) -> int:
    return dim if kind.startswith("poisson") else len(PAIRS[dim])


def voigt_operators(a: Assembled, kind: str, dim: int):
    """(B[e, t, local dof], V[e, t, t], w[t]) of an ``Assembled``: the strain of a local dof in Voigt order with the shear DOUBLED, the
    material on such strains (V s is the flux / stress in Voigt order, shear NOT doubled, so that s . V s is the energy), and the weights
    of the flux norm (|q|^2 = sum_t w_t q_t^2: the Frobenius norm of the stress counts the shear twice)."""
    one, two = a.dtype(1), a.dtype(2)
    if a.bs == 1:
        return np.transpose(a.xi, (0, 2, 1)), a.C, np.full(dim, one)
    ne = a.xi.shape[0]
    B = np.stack([a.xi[:, :, :, k, l] * (one if k == l else two) for k, l in PAIRS[dim]], axis=1).reshape(ne, len(PAIRS[dim]), -1)
    V = np.einsum("mij,eijkl,nkl->emn", a.E, a.C, a.E)
    return B, V, np.array([one if k == l else two for k, l in PAIRS[dim]], dtype=a.dtype)


def voigt_material(kind: str, coef, dim: int, dtype=LD) -> np.ndarray:
    """V[e, t, t] of a coefficient stream (or of a direction: the material is linear in the stream)."""
    C = material_tensor(kind, coef, dim, dtype)
    if kind.startswith("poisson"):
        return C
    E = unit_strains(dim, dtype)
    return np.einsum("mij,eijkl,nkl->emn", E, C, E)


def n_components(kind: str, dim: int) -> int:
    t = dim * (dim + 1) // 2
    return {"poisson": 1, "poisson_matrix": t, "elasticity": 2, "elasticity_voigt": t * (t + 1) // 2}[kind]


def region_rows(vol, s, q, nrm, labels, n_regions: int) -> dict:
    """The region statistics of ``Reconstruction`` from the element fields, in the number format of the fields."""
    labels = np.asarray(labels)
    out = {"region_volume": [], "region_mean_strain": [], "region_mean_flux": [], "region_energy": [], "region_max_flux": [], "region_norm": []}
    for r in range(n_regions):
        sel = labels == r
        v = vol[sel].sum()
        out["region_volume"].append(v)
        out["region_mean_strain"].append(vol[sel] @ s[sel] / v)
        out["region_mean_flux"].append(vol[sel] @ q[sel] / v)
        out["region_energy"].append(vol[sel] @ np.einsum("et,et->e", s[sel], q[sel]))
        out["region_max_flux"].append(nrm[sel].max())
        out["region_norm"].append(np.where(sel, nrm, -1))
    return {k: np.array(v) for k, v in out.items()}


def derived_truth(kind, x, cells, to_periodic, coef, M=None, xi=None, directions=None, weights=None, loads=None, labels=None,
                  solver: str = "refine") -> dict:
    """Everything the package computes from the correctors, in long double and in the package's conventions (those of tests/recon_ref.py,
    sens_ref.py, strat_sens_ref.py, loads_ref.py): Voigt order, strains with the shear doubled, fluxes without, Frobenius flux norm.

    always    A[t, t], chi[n_dof, t] (mean-free), C0[t, t], vol[e], s_canon[t, e, t] (the strain of every canonical load)
    xi[t]     strain / flux [e, t], mean_strain / mean_flux [t], energy, norm[e] (the flux norm), max_flux; with labels[e] the region_* rows
              (mean strain and flux divided by the region's volume, energy not) and region_norm[r, e] (-1 outside the region)
    directions[n, e(, n_comp)]   dA[n, t, t] = sum_K |K| s^m_K . material(dir_K) s^n_K;  d2A[n, n, t, t], the second derivatives along
                                 the directions in the energy form of tests/sens2_ref.py (eps_b[m] the strain of the corrector of the load
                                 material(dir_b) s^m):  -sum_K |K| (eps_b[m] . V(coef) eps_a[n] + eps_a[m] . V(coef) eps_b[n]);  d2A_direct, the
                                 form the library sums (g_ab + g_ab^T, g_ab[m][n] = sum_K |K| eps_b[m] . material(dir_a) s^n): the same number
                                 in exact arithmetic, no sum shared; for the identity check of the host test only
    weights[t, t]                grad[e(, n_comp)] of weights : A_H;  dA_dM[d, d, t, t] (always) and grad_M[d, d] by the moment form
    loads[l, e, t]               load_chi[n_dof, l] (mean-free), P_eff / load_mean_flux [l, t], load_energy[l, l], load_strain / load_flux
                                 [l, e, t], load_norm[l, e], load_max_flux[l]"""
    cells = np.asarray(cells)
    dim = cells.shape[1] - 1
    a = Assembled(kind, x, cells, to_periodic, coef, M, LD)
    t, ne = a.t, cells.shape[0]
    B, V, w = voigt_operators(a, kind, dim)
    vol = a.vol
    rhs = [a.load()]
    if loads is not None:
        P = np.asarray(loads).astype(LD)  # float64 from the tests; long double where a host test needs loads that float64 cannot hold
        F = np.zeros((a.nd, P.shape[0]), dtype=LD)
        np.add.at(F, a.rows.ravel(), -np.einsum("e,eta,let->eal", vol, B, P).reshape(-1, P.shape[0]))
        rhs.append(F)
    sol = solve_ld(a, np.concatenate(rhs, axis=1), solver)
    chi = sol[:, :t]
    s_canon = np.eye(t, dtype=LD)[:, None, :] + np.einsum("eta,eam->met", B, chi[a.rows])
    q_canon = np.einsum("etu,meu->met", V, s_canon)
    out = {"A": a.energy(chi), "chi": a.mean_free(chi), "C0": a.C0, "vol": vol, "s_canon": s_canon}
    if xi is not None:
        xi = np.asarray(xi, dtype=np.float64).astype(LD)
        s, q = np.einsum("m,met->et", xi, s_canon), np.einsum("m,met->et", xi, q_canon)
        nrm = np.sqrt(np.einsum("t,et->e", w, q * q))
        out.update(strain=s, flux=q, mean_strain=vol @ s, mean_flux=vol @ q, energy=vol @ np.einsum("et,et->e", s, q), norm=nrm,
                   max_flux=nrm.max())
        if labels is not None:
            out.update(region_rows(vol, s, q, nrm, labels, int(np.max(labels)) + 1))
    if directions is not None:
        out["dA"] = np.stack([np.einsum("e,met,etu,neu->mn", vol, s_canon, voigt_material(kind, d, dim), s_canon) for d in directions])
        Vd = np.stack([voigt_material(kind, d, dim) for d in directions])
        # the derivative of chi^m along dir_b is the corrector of the load V(dir_b) s^m (tests/sens2_ref.py); a second solve: its
        # right-hand sides are formed from the canonical correctors
        nd = len(Vd)
        Pd = np.einsum("betu,meu->bmet", Vd, s_canon).reshape(nd * t, ne, t)
        Fd = np.zeros((a.nd, nd * t), dtype=LD)
        np.add.at(Fd, a.rows.ravel(), -np.einsum("e,eta,let->eal", vol, B, Pd).reshape(-1, nd * t))
        eps_d = np.einsum("eta,eal->let", B, solve_ld(a, Fd, solver)[a.rows]).reshape(nd, t, ne, t)
        en = np.einsum("e,bmet,etu,aneu->abmn", vol, eps_d, V, eps_d)
        out["d2A"] = -(en + np.transpose(en, (1, 0, 2, 3)))
        gd = np.einsum("e,bmet,aetu,neu->abmn", vol, eps_d, Vd, s_canon)
        out["d2A_direct"] = gd + np.transpose(gd, (0, 1, 3, 2))
    # the stratification: H^n_K[alpha][b] = sum_a chi_n[p_a bs + alpha] g_a[b] (no M), sigma^m_K as a d x bs matrix
    g = element_geometry(x, cells, dim, LD)[0]
    H = np.einsum("eaxn,eab->nexb", chi[a.rows].reshape(ne, dim + 1, a.bs, t), g)
    if a.bs == 1:
        sig = q_canon[..., None]
    else:
        sig = np.zeros((t, ne, dim, dim), dtype=LD)
        for p, (k, l) in enumerate(PAIRS[dim]):
            sig[:, :, k, l] = sig[:, :, l, k] = q_canon[:, :, p]
    half = np.einsum("e,meax,nexb->abmn", vol, sig, H)
    out["dA_dM"] = half + np.swapaxes(half, 2, 3)
    if weights is not None:
        W = np.asarray(weights, dtype=np.float64).astype(LD)
        nc = n_components(kind, dim)
        grad = np.zeros((ne, nc), dtype=LD)
        for c in range(nc):
            unit = np.zeros((ne, nc))
            unit[:, c] = 1.0
            grad[:, c] = vol * np.einsum("mn,met,etu,neu->e", W, s_canon, voigt_material(kind, unit.reshape(ne, -1) if nc > 1 else unit[:, 0], dim),
                                         s_canon)
        out["grad"] = grad if nc > 1 else grad[:, 0]
        out["grad_M"] = np.einsum("mn,abmn->ab", W, out["dA_dM"])
    if loads is not None:
        lchi = sol[:, t:]
        eps = np.einsum("eta,eal->let", B, lchi[a.rows])
        q = P + np.einsum("etu,leu->let", V, eps)
        nrm = np.sqrt(np.einsum("t,let->le", w, q * q))
        Peff = np.einsum("e,let->lt", vol, q)
        out.update(load_chi=a.mean_free(lchi), P_eff=Peff, load_mean_flux=Peff, load_energy=np.einsum("e,let,etu,keu->lk", vol, eps, V, eps),
                   load_strain=eps, load_flux=q, load_norm=nrm, load_max_flux=nrm.max(axis=1))
    return out


CORRECTOR_QUANTITIES = ("chi", "load_chi")  # capped at 1e-10 by the host test; every other derived yardstick at 1e-11
REGION_QUANTITIES = ("region_volume", "region_mean_strain", "region_mean_flux", "region_energy", "region_max_flux")
LOAD_QUANTITIES = ("load_chi", "P_eff", "load_mean_flux", "load_energy", "load_strain", "load_flux", "load_max_flux")


def derived_float64(kind, x, cells, to_periodic, coef, M=None, xi=None, directions=None, weights=None, loads=None, labels=None,
                    n: int | None = None, msh=None) -> dict:
    """The same quantities, under the names of ``derived_truth``, from the EXISTING float64 NumPy references on the same inputs:
    tests/recon_ref.py (correctors of the oracle on the structured cell with ``n`` cells per side, of periodic_fem on ``msh``),
    strat_sens_ref and loads_ref (their own sparse LU, dof order of ``to_periodic``), sens_ref.Cell on the canonical strains of loads_ref."""
    import loads_ref as LR
    import recon_ref as RR
    import sens2_ref as S2
    import sens_ref as SR
    import strat_sens_ref as TR

    cells = np.asarray(cells)
    dim = cells.shape[1] - 1
    t = tensor_size(kind, dim)
    ne = cells.shape[0]
    out = {}
    rec = (lambda v: RR.structured(kind, dim, n, coef, M, v)) if msh is None else (lambda v: RR.on_mesh(msh, kind, coef, M, v))
    if xi is not None:
        r = rec(xi)
        out.update(strain=r["s"], flux=r["q"], mean_strain=r["mean_strain"], mean_flux=r["mean_flux"], energy=r["energy"],
                   max_flux=r["max_flux"], argmax_element=r["argmax_element"])
        if labels is not None:
            wt = np.array([1.0 if (kind.startswith("poisson") or m < dim) else 2.0 for m in range(t)])
            vol = RR._geometry(np.asarray(x, float)[cells][:, :, :dim])[1]
            out.update(region_rows(vol, r["s"], r["q"], np.sqrt((r["q"] ** 2) @ wt), labels, int(np.max(labels)) + 1))
    st = TR.StratCell(x, cells, kind, coef, M, np.asarray(to_periodic))
    # sens_ref's contractions on the canonical strains of loads_ref: sens_ref.structured would solve the oracle's problem once per canonical
    # load for the same strains (1.7 s a cell at 3D elasticity n = 5 against 0.3 s)
    sc = SR.Cell(kind, dim, st.cell.vol, list(st.cell.s_canon), st.cell.A)
    if directions is not None:
        out["dA"] = np.stack([sc.dA(d) for d in directions])
        out["d2A"] = S2.second_derivatives(st.cell, directions)  # the energy form, on the cell of loads_ref built above
    if weights is not None:
        gr = sc.grad(np.asarray(weights, float), n_components(kind, dim))
        out["grad"] = gr if gr.shape[1] > 1 else gr[:, 0]
    out["dA_dM"] = TR.dA_dM(st)
    out["A"], out["chi"] = st.cell.A, st.cell.chi_canon.T
    if weights is not None:
        out["grad_M"] = TR.grad_M(st, weights)
    if loads is not None:
        r = st.cell.solve(loads)
        out.update(load_chi=r["chi"].T, P_eff=r["P_eff"], load_mean_flux=r["P_eff"], load_energy=r["energy"], load_strain=r["eps"],
                   load_flux=r["q"], load_max_flux=r["max_flux"])
    return out


def euler_directions(coef, directions) -> list:
    """The directions that ARE the cell's coefficient.  A_H is homogeneous of degree one in the coefficient, so every block of d2A with such
    a direction vanishes (Euler): the truth holds rounding there (1e-20 of the largest block), and an error relative to the block itself
    means nothing.  Decided from the inputs, never from the size of a result."""
    coef = np.asarray(coef)
    return [k for k, d in enumerate(directions) if np.array_equal(np.asarray(d), coef)]


def block_rel(A, T, euler=()) -> np.ndarray:
    """e[a, b] = max|A[a, b] - T[a, b]| / max|T[a, b]| of d2A[a, b, t, t] per block; the blocks with a or b in ``euler``
    (``euler_directions``) over max|T| of the whole array."""
    T = np.asarray(T, dtype=LD)
    d = np.abs(np.asarray(A, dtype=LD) - T).max(axis=(2, 3))
    scale = np.abs(T).max(axis=(2, 3))
    for k in euler:
        scale[k, :] = scale[:, k] = np.abs(T).max()
    return (d / scale).astype(np.float64)


def derived_float64_errors(kind, x, cells, to_periodic, coef, M=None, xi=None, directions=None, weights=None, loads=None, labels=None,
                           T: dict | None = None, n: int | None = None, msh=None) -> dict:
    """Per quantity  e = max|ref64 - T| / max|T|  over the cell's whole array (T = ``derived_truth``, computed here when None; ref64 =
    ``derived_float64``) and  bound = 32 * max(e, 16 eps):  {"e": {name: e}, "bound": {name: bound}}.  Never from a GPU result.
    d2A PER BLOCK: e["d2A"] and bound["d2A"] are [n_dirs, n_dirs] arrays (``block_rel`` with the ``euler_directions`` of the inputs): the
    blocks differ by three orders of magnitude, so the whole-array error would hide a loss in the small ones."""
    if T is None:
        T = derived_truth(kind, x, cells, to_periodic, coef, M, xi, directions, weights, loads, labels)
    ref = derived_float64(kind, x, cells, to_periodic, coef, M, xi, directions, weights, loads, labels, n=n, msh=msh)
    e = {k: rel(v, T[k]) for k, v in ref.items() if k in T and k not in ("region_norm", "d2A")}
    b = {k: bound(v, 0.0) for k, v in e.items()}
    if "d2A" in ref:
        e["d2A"] = block_rel(ref["d2A"], T["d2A"], euler_directions(coef, directions))
        b["d2A"] = FACTOR * np.maximum(e["d2A"], FLOOR_EPS * EPS)
    return {"e": e, "bound": b}


# ------------------------------------------------------------------------------------------------------------------------------
# coefficient families and cases of the GPU accuracy tests
# ------------------------------------------------------------------------------------------------------------------------------

FAMILIES = {"poisson": ("log2", "tp4", "tp7"), "poisson_matrix": ("log2", "tp4", "tp7"), "elasticity": ("log2", "tp5"),
            "elasticity_voigt": ("log2", "tp5")}


def _spd_stream(rng, nc, ne, m, pairs):
    L = np.eye(m) + 0.3 * rng.standard_normal((nc, ne, m, m))
    S = L @ np.swapaxes(L, -1, -2)
    return np.stack([S[..., k, l] for k, l in pairs], axis=-1)


def coefficients(kind: str, dim: int, ne: int, family: str, nc: int, seed: int) -> np.ndarray:
    """coef[nc, ne(, n_comp)] of a family, geometric mean of order one:

    log2  log-uniform over two decades                    tp4 / tp5 / tp7  random two-phase, contrast 1e4 / 1e5 / 1e7
    The scalar field multiplies a fixed random SPD matrix per element for the matrix-valued kinds; isotropic elasticity takes the
    field in both Lame parameters (independent log-uniform draws, one shared phase mask: the C4 fibre contrast).

    The stiff phase fills 70 % of the elements, so that it percolates and A_H is of the order of the arithmetic mean C0.  In a soft-dominated
    mixture A_H << C0 and EVERY float64 evaluation of C0 - B^T K^-1 B loses contrast x eps to the cancellation (measured: 3e-11 at 1e5 on 2D
    elasticity n = 25); the bound would follow the yardstick there, but the host test keeps the yardstick itself below 1e-12."""
    rng = np.random.default_rng(seed)
    if family == "log2":
        s = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=(nc, ne)))
        s2 = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=(nc, ne)))
    else:
        c = 10.0 ** int(family[2:])
        s = np.where(rng.random((nc, ne)) < 0.7, np.sqrt(c), 1.0 / np.sqrt(c))
        s2 = 0.5 * s
    if kind == "poisson":
        return s
    if kind == "elasticity":
        return np.stack([s, s2], axis=-1)
    if kind == "poisson_matrix":
        return s[..., None] * _spd_stream(rng, nc, ne, dim, PAIRS[dim])
    t = dim * (dim + 1) // 2
    iu = np.triu_indices(t)
    return s[..., None] * _spd_stream(rng, nc, ne, t, list(zip(iu[0], iu[1])))


def stratification(dim: int, nc: int, seed: int) -> np.ndarray:
    return np.eye(dim)[None] + 0.3 * np.random.default_rng(seed + 7919).standard_normal((nc, dim, dim))


def rotation(dim: int, angle: float) -> np.ndarray:
    """The plane rotation by ``angle``; in 3D the rotation by it about (1, 1, 1) (Rodrigues)."""
    c, s = np.cos(angle), np.sin(angle)
    if dim == 2:
        return np.array([[c, -s], [s, c]])
    u = np.ones(3) / np.sqrt(3.0)
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return c * np.eye(3) + s * Kx + (1 - c) * np.outer(u, u)


M_FAMILIES = ("mild", "shear30", "squeeze16", "rot")


def stratification_family(name: str, dim: int, nc: int, seed: int, shear: float = 30.0, squeeze: float = 16.0) -> np.ndarray:
    """M[nc, d, d] of a family.  mild: I + 0.3 N (``stratification``); shear30: I + 30 e_0 e_{d-1}^T; squeeze16: rot(0.3) diag(1, 1/16[, 1]);
    rot: rot(0.7).  Only ``mild`` differs between the cells.  ``shear`` / ``squeeze``: softened values for a case whose float64 yardstick
    would pass a cap of tests/test_accuracy_ref_host.py otherwise."""
    if name == "mild":
        return stratification(dim, nc, seed)
    if name == "shear30":
        M = np.eye(dim)
        M[0, dim - 1] += shear
    elif name == "squeeze16":
        D = np.ones(dim)
        D[1] = 1.0 / squeeze
        M = rotation(dim, 0.3) @ np.diag(D)
    elif name == "rot":
        M = rotation(dim, 0.7)
    else:
        raise ValueError(name)
    return np.repeat(M[None], nc, axis=0)


# (route asserted through plan.kernel, kind, dim, n, plan flags).  The smallest shapes that reach each code path.
STRUCTURED_CASES = {
    # default plans
    "default": [
        ("fused2d", "poisson", 2, 5, 0), ("fused2d", "poisson", 2, 16, 0), ("fused2d", "poisson", 2, 17, 0), ("fused2d", "poisson", 2, 32, 0),
        ("small_wave", "poisson", 3, 4, 0), ("small_wave", "elasticity", 2, 10, 0), ("small_wave", "elasticity", 3, 3, 0),
        ("small_wave", "poisson", 3, 6, 0), ("small_wave", "elasticity", 3, 4, 0), ("small_wave", "poisson_matrix", 2, 12, 0),
        ("small_wave", "elasticity_voigt", 2, 7, 0),
        ("small_fused", "poisson", 3, 7, 0), ("small_fused", "poisson", 3, 8, 0),
        ("multifrontal", "elasticity", 2, 25, 0), ("multifrontal", "elasticity", 3, 5, 0), ("multifrontal", "poisson", 3, 9, 0),
    ],
    # HOMMX_MF_STAGE=64: the staged elimination of the tree's large fronts
    "staged": [("multifrontal", "elasticity", 2, 25, 0), ("multifrontal", "elasticity", 3, 5, 0), ("multifrontal", "poisson", 3, 9, 0)],
    # HOMMX_NO_SMALL_FUSED=1 HOMMX_MF_MIN_B=0: the plane elimination (one 64 leaf; padded 96 = the 32 + 64 recursion; forced 2D)
    "plane": [("blocked", "poisson", 3, 6, 0), ("blocked", "elasticity", 3, 4, 0), ("blocked", "elasticity", 3, 5, 0),
              ("blocked", "poisson", 3, 9, 0), ("blocked", "poisson", 2, 16, 1)],
}
CHILD_ENV = {"default": {}, "staged": {"HOMMX_MF_STAGE": "64"}, "plane": {"HOMMX_NO_SMALL_FUSED": "1", "HOMMX_MF_MIN_B": "0"},
             # derived outputs only: the load solves of the fused 2D plans by one more elimination of the blocked family
             "blocked_loads": {"HOMMX_FUSED_LOADS": "0"}}
# (kernel, kind, mesh builder name, builder arguments, route)
MESH_CASES = [
    ("mesh_front", "elasticity", "jittered_unit_square", (9, 7), None), ("mesh_front", "poisson", "jittered_unit_cube", (3, 4, 3), None),
    ("mesh_multifrontal", "elasticity", "jittered_unit_square", (9, 7), "tree"),
    ("mesh_multifrontal", "poisson", "jittered_unit_cube", (3, 4, 3), "tree"),
]
# (corrector kernel, kind, dim, n, group): fused2d_subst; plane elimination behind a small-block plan; the tree's back substitution
CORRECTOR_CASES = [("fused2d_subst", "poisson", 2, 16, "default"), ("fused2d_subst", "poisson", 2, 32, "default"),
                   ("blocked", "poisson", 3, 6, "default"), ("multifrontal", "elasticity", 3, 5, "default")]
# one mild-contrast case per kernel family for the magnitude sweep: (group, kernel, kind, dim, n, flags) or a mesh case
SWEEP_K = (-40, -20, 0, 20, 30, 40)
SWEEP_CASES = [("default", "fused2d", "poisson", 2, 16, 0), ("default", "fused2d", "poisson", 2, 32, 0),
               ("default", "small_wave", "elasticity", 2, 10, 0), ("default", "small_fused", "poisson", 3, 7, 0),
               ("default", "multifrontal", "elasticity", 3, 5, 0), ("plane", "blocked", "poisson", 3, 6, 0)]
SWEEP_MESH = MESH_CASES[0]
# correctors and user-supplied loads under the magnitude sweep (default plans): the three corrector paths -- substitution on the fused
# kernel's records, the plane elimination behind a small-block plan, the tree's back substitution
SWEEP_LOAD_CASES = [("poisson", 2, 16), ("elasticity", 2, 10), ("elasticity", 3, 5)]
SWEEP_LOAD_K = (-40, 0, 40)
NC = 2


def case_seed(*key) -> int:
    import zlib

    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def structured_inputs(kind, dim, n, family, with_M):
    """(coef[NC, ...], M[NC, d, d] or None) of a structured case: seeded by the case itself."""
    ne = (2 if dim == 2 else 6) * n**dim
    seed = case_seed(kind, dim, n, family)
    return coefficients(kind, dim, ne, family, NC, seed), (stratification(dim, NC, seed) if with_M else None)


def load_inputs(kind, dim, n):
    """P[2, n_el, t]: two seeded polarisation fields of order one, shared by the cells of the case."""
    ne = (2 if dim == 2 else 6) * n**dim
    t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
    return np.random.default_rng(case_seed("loads", kind, dim, n)).standard_normal((2, ne, t))


def mesh_of(builder: str, args):
    from hommx_amd import workloads as W

    return getattr(W, builder)(*args)


def mesh_inputs(kind, builder, args, family, with_M):
    msh = mesh_of(builder, args)
    seed = case_seed(kind, builder, args, family)
    dim = msh.topology.dim
    return msh, coefficients(kind, dim, msh.num_cells, family, NC, seed), (stratification(dim, NC, seed) if with_M else None)


# ------------------------------------------------------------------------------------------------------------------------------
# the stratification on the tensor routes, and the derived outputs (tests/test_gpu_accuracy.py, tests/test_gpu_accuracy_derived.py)
# ------------------------------------------------------------------------------------------------------------------------------

# one case per kernel family, and the padded fused blocks: (group, kernel, kind, dim, n, flags) or (group,) + a mesh case
M_CASES = list(SWEEP_CASES) + [("default", "fused2d", "poisson", 2, 5, 0), ("default", "fused2d", "poisson", 2, 17, 0),
                               ("default",) + MESH_CASES[0], ("default",) + MESH_CASES[2]]
M_CONDITIONING = ("shear30", "squeeze16", "rot")
M_SCALES = ((0, 0), (0, 8), (0, -8), (0, 20), (0, -20), (40, -20), (-40, 20), (40, 20), (-40, -20))  # (k, j): coef * 2^k, M * 2^j
# (case id, coefficient family, M family) -> softened parameter of ``stratification_family``.  The 2D Poisson cells at contrast 1e7 under
# shear 30: the long-double refinement of ``truth`` stalls above STALL_LIMIT on the second cell (n = 16: 4.3e-14, n = 32: 8.4e-15, n = 17:
# 1.2e-15), so there is no truth to test against; at shear 8 it converges and the yardsticks stay below 1e-13 (correctors 2.2e-12).
# log2 keeps shear 30 on these cases, and n = 5 keeps it on both families.
SOFTENED = {(f"fused2d-poisson-2-{n}", "tp7", "shear30"): {"shear": 8.0} for n in (16, 17, 32)}


def top_family(kind: str) -> str:
    return FAMILIES[kind][-1]


def is_mesh_case(case) -> bool:
    """Of a case without its group: (kernel, kind, builder, args, route) rather than (kernel, kind, dim, n[, flags])."""
    return isinstance(case[2], str)


def case_id(case) -> str:
    """Of (kernel, kind, dim, n[, flags]) or (kernel, kind, builder, args, route)."""
    if is_mesh_case(case):
        return f"{case[0]}-{case[1]}-{case[2]}{'x'.join(map(str, case[3]))}"
    return "-".join(map(str, case[:4])) + ("-forced" if len(case) > 4 and case[4] else "")


def case_inputs(case, family: str, m_family: str | None):
    """(coef[NC, ...], M[NC, d, d] or None, geometry) of a structured or mesh case (without its group) with M from a family: the
    coefficients of ``structured_inputs`` / ``mesh_inputs``.  geometry = dict(x, cells, tp, kw) with kw what ``float64_errors`` takes."""
    if is_mesh_case(case):
        _, kind, builder, args, _ = case
        msh, coef, _ = mesh_inputs(kind, builder, args, family, False)
        x, cells, tp = mesh_arrays(msh)
        dim, seed, kw = msh.topology.dim, case_seed(kind, builder, args, family), {"msh": msh}
    else:
        _, kind, dim, n = case[:4]
        coef, _ = structured_inputs(kind, dim, n, family, False)
        x, cells, tp = structured(dim, n)
        seed, kw = case_seed(kind, dim, n, family), {"n": n}
    M = None if m_family is None else stratification_family(m_family, dim, NC, seed, **SOFTENED.get((case_id(case), family, m_family), {}))
    return coef, M, {"x": x, "cells": cells, "tp": tp, "kw": kw}


# (kernel, corrector kernel, kind, dim, n) and (kernel, corrector kernel, kind, builder, args, route): the smallest shapes that reach
# every (dim, kind, mesh) instantiation of the reconstruction, sensitivity and load kernels, on every corrector source
DERIVED_CASES = [
    ("fused2d", "fused2d_subst", "poisson", 2, 16),  # NB = 16
    ("fused2d", "fused2d_subst", "poisson", 2, 17),  # NB = 32, padded; 578 elements
    ("small_wave", "blocked", "elasticity", 2, 10),  # plane correctors
    ("small_wave", "blocked", "poisson", 3, 6),
    ("small_wave", "blocked", "poisson_matrix", 2, 12),  # full-tensor instantiations
    ("small_wave", "blocked", "elasticity_voigt", 2, 7),
    ("multifrontal", "multifrontal", "elasticity", 3, 5),  # tree back substitution; 750 elements, no multiple of a block
    ("mesh_front", "mesh_front", "elasticity", "jittered_unit_square", (9, 7), None),
    ("mesh_multifrontal", "mesh_multifrontal", "poisson", "jittered_unit_cube", (3, 4, 3), "tree"),
]
# (coefficient family or None for the kind's top-contrast family, M family or None)
DERIVED_FAMILIES = (("log2", None), ("log2", "mild"), (None, "mild"), ("log2", "shear30"), ("log2", "squeeze16"))
DERIVED_SWEEP_CASES = [DERIVED_CASES[0], DERIVED_CASES[2], DERIVED_CASES[6], DERIVED_CASES[7]]  # one per corrector path
DERIVED_SWEEP_KJ = ((0, 0), (40, 0), (-40, 0), (0, 20), (0, -20), (40, -20), (-40, 20))
# the power (of 2^k, of 2^j) by which every derived output scales under coef * 2^k, M * 2^j, loads * 2^k with xi, directions and weights
# fixed: decided by test_scaling_laws_are_exact of tests/test_accuracy_ref_host.py
SCALING_LAWS = {
    "A": (1, 0), "chi": (0, -1), "strain": (0, 0), "flux": (1, 0), "mean_strain": (0, 0), "mean_flux": (1, 0), "energy": (1, 0),
    "max_flux": (1, 0), "region_volume": (0, 0), "region_mean_strain": (0, 0), "region_mean_flux": (1, 0), "region_energy": (1, 0),
    "region_max_flux": (1, 0), "dA": (0, 0), "grad": (0, 0), "dA_dM": (1, -1), "grad_M": (1, -1), "load_chi": (0, -1), "P_eff": (1, 0),
    "load_mean_flux": (1, 0), "load_energy": (1, 0), "load_strain": (0, 0), "load_flux": (1, 0), "load_max_flux": (1, 0),
    "d2A": (-1, 0), "d2A_direct": (-1, 0),
}
# the third sweep: directions * 2^i with everything else fixed, at (k, j) = (0, 0).  The power of 2^i by which dA and d2A scale (linear and
# bilinear in the directions); decided by the same host test
DERIVED_SWEEP_DIR = (-20, 20)
DIRECTION_LAWS = {"dA": 1, "d2A": 2, "d2A_direct": 2}


def derived_case(case):
    """(kernel, corrector kernel, the case as ``case_inputs`` takes it)."""
    return case[0], case[1], (case[0],) + tuple(case[2:])


def derived_inputs(case, coef0: np.ndarray) -> dict:
    """The fixed seeded inputs of a derived case, shared by its cells: xi[t], three directions (the cell-0 coefficient ``coef0``, a random
    stream, the indicator of every other element), weights[t, t], two loads of order one, two-region labels (both regions occupied)."""
    _, kind = case[:2]
    dim = (2 if case[2] == "jittered_unit_square" else 3) if is_mesh_case(case) else case[2]
    t, ne = tensor_size(kind, dim), coef0.shape[0]
    rng = np.random.default_rng(case_seed("derived", case_id(case)))
    every_other = np.zeros_like(coef0)
    every_other[::2] = 1.0
    labels = (rng.random(ne) < 0.4).astype(np.uint8)
    labels[:2] = (0, 1)
    return {"xi": rng.standard_normal(t), "directions": np.stack([coef0, rng.standard_normal(coef0.shape), every_other]),
            "weights": rng.standard_normal((t, t)), "loads": rng.standard_normal((2, ne, t)), "labels": labels}
