"""Test-side NumPy reference of the consistent tangent of the secant response (include/hommx_hip.h, hommx_secant_tangent_source;
DESIGN.md 4.16), one cell at a time: ``secant_ref.iterate``, then the element tangent

    T_K = material(c_K) + sum_k (material(unit_k) e_K) (dL_k/de)^T

from the ANALYTIC derivative of the law, written here per law and per kind in plain NumPy (nothing of ``SecantLaw.host_tangent``, of
``_run``'s forward mode or of the tangent rules is used), then the solver of ``recon_ref`` on the tangent kind with the symmetric part
of T as its coefficient: D = A_eff of that linear cell problem.

The potential laws of the tests, each with a symmetric T by construction (phi(s) = 0.5 + 0.5 / (1 + s), psi(s) = 0.5 / (1 + s)):
  poisson            c[0] phi(|e|^2), the full |e|^2 in 3D
  poisson_matrix     the diagonal entries c[k] + psi(|e|^2), the others copied
  elasticity         lam = c[0], mu = c[1] phi(eps:eps), eps:eps = sum normal^2 + 0.5 sum shear^2 (e holds the doubled shear)
  elasticity_voigt   the diagonal entry of row r is c[k] + 0.5 / (1 + e[r]^2), the others copied
and ASYMMETRIC, the mu law with the shear term counted twice as much (``e2^2`` for ``0.5 e2^2``): no potential.
"""

from __future__ import annotations

import numpy as np

import periodic_fem as PF
import recon_ref as R
import secant_ref as S

N_COMP = {"poisson": lambda d: 1, "poisson_matrix": lambda d: d * (d + 1) // 2, "elasticity": lambda d: 2,
          "elasticity_voigt": lambda d: 21 if d == 3 else 6}
TANGENT_KIND = {"poisson": "poisson_matrix", "poisson_matrix": "poisson_matrix", "elasticity": "elasticity_voigt",
                "elasticity_voigt": "elasticity_voigt"}


def tensor_size(kind, dim):
    return dim if kind.startswith("poisson") else dim * (dim + 1) // 2


def entries(kind, dim):
    """(r, c), r <= c, of every entry of the coefficient of the matrix and the Voigt kind, in the order of the ABI."""
    t = tensor_size(kind, dim)
    if kind == "poisson_matrix":
        return [(0, 0), (1, 1), (0, 1)] if dim == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    return [(m, n) for m in range(t) for n in range(m, t)]


def _sq(terms):
    return " + ".join(terms)


def potential_law(kind, dim, asymmetric=False):
    """(SecantLaw, dlaw): the law of the module docstring and dlaw(e[n_el, t], b[n_el, n_comp]) -> dc/de[n_el, n_comp, t], by hand."""
    from hommx_amd.expr import SecantLaw

    t = tensor_size(kind, dim)
    if kind == "poisson":
        s = _sq([f"e[{i}]**2" for i in range(t)])
        law = SecantLaw(f"c[0]*(0.5 + 0.5/(1 + {s}))")

        def dlaw(e, b):
            g = 1.0 + (e ** 2).sum(1)
            return (b[:, 0, None] * (-0.5 / g[:, None] ** 2) * 2.0 * e)[:, None, :]

    elif kind == "poisson_matrix":
        s = _sq([f"e[{i}]**2" for i in range(t)])
        diag = [f"c[{k}] + 0.5/(1 + {s})" for k in range(dim)]
        off = {(r, c): f"c[{k}]" for k, (r, c) in enumerate(entries(kind, dim)) if r != c}
        law = SecantLaw([[diag[i] if i == j else off[(min(i, j), max(i, j))] for j in range(dim)] for i in range(dim)])

        def dlaw(e, b):
            g = 1.0 + (e ** 2).sum(1)
            d = np.zeros((len(e), N_COMP[kind](dim), t))
            d[:, :dim, :] = ((-0.5 / g[:, None] ** 2) * 2.0 * e)[:, None, :]
            return d

    elif kind == "elasticity":
        w = 1.0 if asymmetric else 0.5
        s = _sq([f"e[{i}]**2" for i in range(dim)] + [(f"e[{i}]**2" if asymmetric else f"0.5*e[{i}]**2") for i in range(dim, t)])
        law = SecantLaw(lam="c[0]", mu=f"c[1]*(0.5 + 0.5/(1 + {s}))")
        weight = np.array([1.0] * dim + [w] * (t - dim))

        def dlaw(e, b):
            g = 1.0 + (weight * e ** 2).sum(1)
            d = np.zeros((len(e), 2, t))
            d[:, 1, :] = b[:, 1, None] * (-0.5 / g[:, None] ** 2) * 2.0 * weight * e
            return d

    else:
        ent = entries(kind, dim)
        law = SecantLaw([f"c[{k}] + 0.5/(1 + e[{r}]**2)" if r == c else f"c[{k}]" for k, (r, c) in enumerate(ent)])

        def dlaw(e, b):
            d = np.zeros((len(e), len(ent), t))
            for k, (r, c) in enumerate(ent):
                if r == c:
                    d[:, k, r] = -0.5 * 2.0 * e[:, r] / (1.0 + e[:, r] ** 2) ** 2
            return d

    return law, dlaw


def material(kind, dim, c):
    """C[n_el, t, t] in the basis of the canonical loads (the strain with doubled shear), from the tensors of periodic_fem."""
    c = np.asarray(c, float).reshape(len(c), -1)
    C = PF.material_tensor(kind, c, dim)
    if kind.startswith("poisson"):
        return C
    return np.stack([np.stack([C[:, k, l, p, q] for (p, q) in PF.PAIRS[dim]], axis=1) for (k, l) in PF.PAIRS[dim]], axis=1)


def element_tangent(kind, dim, e, cur, base, dlaw):
    """T[n_el, t, t] (not symmetrised) by the formula of the module docstring; material(unit_k) by linearity of ``material``."""
    n_el, n_comp = len(e), N_COMP[kind](dim)
    cur, base = np.asarray(cur, float).reshape(n_el, -1), np.asarray(base, float).reshape(n_el, -1)
    T = material(kind, dim, cur).copy()
    dc = dlaw(e, base)
    zero = material(kind, dim, np.zeros((1, n_comp)))[0]
    for k in range(n_comp):
        unit = material(kind, dim, np.eye(n_comp)[k][None])[0] - zero
        T += np.einsum("mn,en->em", unit, e)[:, :, None] * dc[:, k, None, :]
    return T


def tangent_stream(kind, dim, T):
    """The symmetric T[n_el, t, t] as an element stream of the tangent kind."""
    return np.stack([T[:, r, c] for r, c in entries(TANGENT_KIND[kind], dim)], axis=-1)


def tangent(kind, dim, law, dlaw, base, xi, M=None, n=None, msh=None, **kw) -> dict:
    """The iteration of one cell and its consistent tangent: the dict of ``secant_ref.iterate`` and ``T`` (symmetrised), ``asymmetry``,
    ``D``."""
    r = S.iterate(S.solver(kind, dim, n, msh), law, base, xi, M=M, **kw)
    T = element_tangent(kind, dim, r["s"], r["coef"], base, dlaw)
    top = np.abs(T).max()
    r["asymmetry"] = 0.0 if top == 0.0 else np.abs(T - T.transpose(0, 2, 1)).max() / top
    r["T"] = 0.5 * (T + T.transpose(0, 2, 1))
    r["D"] = S.solver(TANGENT_KIND[kind], dim, n, msh)(tangent_stream(kind, dim, r["T"]), M, xi)["A"]
    return r
