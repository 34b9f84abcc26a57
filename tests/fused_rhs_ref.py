"""NumPy statement of the extended factor record of a 2D scalar cell and of the solve for ANY compatible right-hand side on it (DESIGN 4.8,
4.10): what k_poisson2d_fused<NB, true> records and k_fused2d_subst_rhs evaluates.  Builds on fused_subst_ref (same notation, positive
convention): the record gains N_last, the inverse of the last Schur block after the gauge (last row and column zero, diagonal 1), and
loses what belonged to the canonical loads (nt, x_last), which the solve forms itself:
    A  forward    rt_0 = r_0;  nt_j = N_j rt_j;  rt_{j+1} = r_{j+1} - E_j nt_j                         (j < n-2)
    B  backward   h = nt_{n-2};  h = nt_j - N_j E_j^T h  (j = n-3 .. 0)                                Horner form of sum_j W_j nt_j = C h
       last row   r_last = r_{n-1} - C h - E_{n-2} nt_{n-2};  r_last[last] = 0;  x_last = N_last r_last
    C, D          fused_subst_ref.substitute on these nt and x_last
`device_solve` is the same with the signs, the two-vector couplings and the magnitude exponent the kernel carries."""

import numpy as np

import fused_subst_ref as F


def dense_stiffness(cell) -> np.ndarray:
    """K of a loads_ref.Cell (scalar: one dof per node), dense."""
    nl = cell.rows.shape[1]
    Ke = np.einsum("e,eta,etu,eub->eab", cell.vol, cell.B, cell.V, cell.B)
    K = np.zeros((cell.nd, cell.nd))
    np.add.at(K, (np.repeat(cell.rows, nl, axis=1).ravel(), np.tile(cell.rows, (1, nl)).ravel()), Ke.ravel())
    return K


def factor(K, n):
    """The extended record: N[j] = S_j^-1, E[j] (j = 0 .. n-2), C, N_last.  fused_subst_ref.factor run on the loads [0; ...; 0; I]: every
    nt_j vanishes, r_last = I with its gauged row zeroed, so x_last is N_last but for the gauged diagonal entry."""
    B = np.zeros((n * n, n))
    B[(n - 1) * n:] = np.eye(n)
    f = F.factor(K, B, n)
    N_last = f["x_last"].copy()
    N_last[-1, -1] = 1.0
    return dict(N=f["N"], E=f["E"], C=f["C"], N_last=N_last)


def solve(rec, r, n):
    """x[n n, loads] with K x = r (gauge: the last unknown is 0; not centred), r[n n, loads] compatible."""
    N, E, C = rec["N"], rec["E"], rec["C"]
    r = np.asarray(r, float).reshape(n * n, -1)
    rj = [r[j * n:(j + 1) * n] for j in range(n)]
    nt, rt = [], rj[0]
    for j in range(n - 1):  # A
        nt.append(N[j] @ rt)
        if j < n - 2:
            rt = rj[j + 1] - E[j] @ nt[j]
    h = nt[n - 2]
    for j in range(n - 3, -1, -1):  # B
        h = nt[j] - N[j] @ (E[j].T @ h)
    r_last = rj[n - 1] - C @ h - E[n - 2] @ nt[n - 2]
    r_last[-1] = 0.0
    return F.substitute(dict(N=N, nt=nt, E=E, C=C, x_last=rec["N_last"] @ r_last), n)


def correctors(rec, f, n):
    """Mean-free chi[n n, loads] with K chi = -f."""
    chi = solve(rec, -np.asarray(f, float).reshape(n * n, -1), n)
    return chi - chi.mean(axis=0, keepdims=True)


# -- the device's form ---------------------------------------------------------------------------------------------------------------------
def _two_vectors(E):
    """e0[i] = E[i][i], e1[i] = E[i][i-1] (cyclic) of a coupling block, which has no other entry."""
    n = len(E)
    i = np.arange(n)
    rest = E.copy()
    rest[i, i] = 0.0
    rest[i, i - 1] = 0.0
    assert not rest.any()
    return E[i, i].copy(), E[i, i - 1].copy()


def _mul_E(e, y):
    return e[1][:, None] * np.roll(y, 1, axis=0) + e[0][:, None] * y


def _mul_ET(e, y):
    return e[0][:, None] * y + np.roll(e[1][:, None] * y, -1, axis=0)


def device_record(K, n, esh):
    """The record as the device keeps it, without the padding: of K' = 2^-esh K, N' = -S^-1, every coupling as its two vectors, the header's
    coupling E_{n-1} = C^T, and esh."""
    rec = factor(np.ldexp(np.asarray(K, float), -esh), n)
    return dict(Nn=[-Nj for Nj in rec["N"]], e=[_two_vectors(Ej) for Ej in rec["E"]], c=_two_vectors(rec["C"].T), Nn_last=-rec["N_last"], esh=esh)


def device_correctors(d, f, n):
    """k_fused2d_subst_rhs step by step (y = -x): mean-free chi[n n, loads] with K chi = -f."""
    Nn, e, c = d["Nn"], d["e"], d["c"]
    r = np.ldexp(-np.asarray(f, float).reshape(n * n, -1), -d["esh"])
    rj = [r[j * n:(j + 1) * n] for j in range(n)]
    v, rt = [], rj[0]
    for j in range(n - 1):  # A
        v.append(Nn[j] @ rt)
        rt = rj[j + 1] + _mul_E(e[j], v[j])
    g = v[n - 2]
    for j in range(n - 3, -1, -1):  # B
        g = v[j] + Nn[j] @ _mul_ET(e[j], g)
    rl = rt + _mul_ET(c, g)
    rl[-1] = 0.0
    yl = d["Nn_last"] @ rl
    w, ws = _mul_E(c, yl), []
    for j in range(n - 1):  # C
        if j == n - 2:
            w = w + _mul_ET(e[j], yl)
        ws.append(w)
        w = _mul_E(e[j], Nn[j] @ w)
    y = [None] * n
    y[n - 1] = yl
    for j in range(n - 2, -1, -1):  # D
        q = ws[j] + (_mul_ET(e[j], y[j + 1]) if j < n - 2 else 0.0)
        y[j] = v[j] + Nn[j] @ q
    chi = -np.vstack(y)
    return chi - chi.mean(axis=0, keepdims=True)
