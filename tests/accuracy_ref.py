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
    """A[e, d, d] (Poisson kinds) or C[e, d, d, d, d] (elasticity kinds) in ``dtype`` from the float64 coefficient stream of the C ABI."""
    coef = np.asarray(coef, dtype=np.float64).astype(dtype)
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


def truth(kind, x, cells, to_periodic, coef, M=None, solver: str = "refine"):
    """(A_H[t, t], mean-free correctors[n_dof, t]) in long double; dof = periodic node * bs + component.

    solver='dense': long-double Cholesky of the system with node 0 pinned (N <~ 400).
    solver='refine': float64 sparse LU of the same system, refined with long-double residuals until the correction is below 1e-17 of
    the solution (max norm)."""
    a = Assembled(kind, x, cells, to_periodic, coef, M, LD)
    B = a.load()
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
CHILD_ENV = {"default": {}, "staged": {"HOMMX_MF_STAGE": "64"}, "plane": {"HOMMX_NO_SMALL_FUSED": "1", "HOMMX_MF_MIN_B": "0"}}
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
