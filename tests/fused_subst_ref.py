"""NumPy statement of the block-cyclic-tridiagonal elimination of a 2D scalar cell and of the substitution on its stored block inverses
(DESIGN 4.8): what k_poisson2d_fused<NB, true> records and k_fused2d_subst evaluates, in the positive convention of DESIGN 2, on plain
dense blocks.  Block j = node row j of the n x n torus (dof = i + n j); D_j the diagonal blocks, E_j = K[(., j+1), (., j)],
C = K[(., n-1), (., 0)] the wrap coupling, r_j the loads."""

import numpy as np


def factor(K, B, n):
    """Forward pass.  Returns what the substitution reads, and nothing else: N[j] = S_j^-1, nt[j] = N_j r~_j, E[j] (j = 0 .. n-2), C and
    x_last (gauge: the last unknown is dropped)."""
    K = np.asarray(K.todense() if hasattr(K, "todense") else K, dtype=float)
    blk = lambda a, b: K[a * n:(a + 1) * n, b * n:(b + 1) * n].copy()
    r = [np.array(B[j * n:(j + 1) * n], dtype=float) for j in range(n)]
    E = [blk(j + 1, j) for j in range(n - 1)]
    C = blk(n - 1, 0)
    S, W, rt = blk(0, 0), C.copy(), r[0].copy()
    S_last, r_last = blk(n - 1, n - 1), r[n - 1].copy()
    N, nt = [], []
    for j in range(n - 1):
        if j == n - 2:  # the last row couples to row n-2 through E as well as through the arrow
            W = W + E[j]
        Nj = np.linalg.inv(S)
        N.append(Nj)
        nt.append(Nj @ rt)
        S_last -= W @ Nj @ W.T
        r_last -= W @ nt[j]
        if j < n - 2:
            S = blk(j + 1, j + 1) - E[j] @ Nj @ E[j].T
            W = -W @ Nj @ E[j].T
            rt = r[j + 1] - E[j] @ nt[j]
    S_last[-1, :] = 0.0
    S_last[:, -1] = 0.0
    S_last[-1, -1] = 1.0
    r_last[-1] = 0.0
    return dict(N=N, nt=nt, E=E, C=C, x_last=np.linalg.solve(S_last, r_last))


def substitute(f, n):
    """x[n n, t] from the record of `factor`: the forward u / w sweep (w_j = W_j^T x_last without any W_j), the backward x sweep; not
    centred."""
    N, nt, E, x_last = f["N"], f["nt"], f["E"], f["x_last"]
    w = f["C"].T @ x_last
    u = []
    for j in range(n - 1):
        if j == n - 2:
            w = w + E[j].T @ x_last
        u.append(N[j] @ w)
        if j < n - 2:
            w = -E[j] @ u[j]
    x = [None] * n
    x[n - 1] = x_last
    for j in range(n - 2, -1, -1):
        x[j] = nt[j] - u[j]
        if j < n - 2:  # at j = n-2 the E term is inside W
            x[j] = x[j] - N[j] @ (E[j].T @ x[j + 1])
    return np.vstack(x)


def correctors(K, B, n):
    """Mean-free solutions of K chi = B, [n n, t]."""
    chi = substitute(factor(K, B, n), n)
    return chi - chi.mean(axis=0, keepdims=True)
