"""The two solver-class problems of tests/test_load_sources_hmm_host.py (stand-in plans, CPU) and tests/test_gpu_load_sources.py (the
device): a thermal eigenstrain E(x, y) = alpha(y) dT(x) written once as a vector ``Expression`` whose field ``dT`` is one value per macro
cell, and once as the callable of the eigenstress -A : E that a user had to write by hand before ``set_eigenstrain``.

Both coefficients are ``TwoPhase``: its rule is the centroid rule, so the element mean of the product A E is the product of the element
means and the two statements describe the same discrete load.  The eigenstrain holds one transcendental function of the fast variable.
"""

import numpy as np

from hommx_amd import fem, hmm, mesh, workloads as W
from hommx_amd.expr import Expression

# |u(Expression eigenstrain) - u(callable eigenstress)| / |u| and the same of the effective polarisation, measured ON THE CPU on these
# very problems between the host interpreter of the expression (a stand-in plan: the expression sampled like a callable, the eigenstress
# formed by hmm.eigenstress) and the callable: 0 for the Poisson problem, 1.8e-16 for the elasticity one, recorded here as one unit
# roundoff, below which a relative difference measures nothing.  test_load_sources_hmm_host.py measures them again on every run and fails
# when they exceed this figure; the device tests allow ten times as much.
CPU_DIFFERENCE = {"poisson": 2.0 ** -52, "elasticity": 2.0 ** -52}


def dT(x):
    """The temperature change of a macro cell, read at its midpoint."""
    return 1.0 + 0.5 * x[0] - 0.25 * x[1]


def _alpha(y):
    return 0.01 * (1.0 + 0.5 * np.sin(2 * np.pi * y[0]))


ALPHA = "0.01*(1.0 + 0.5*sin(2*pi*y[0]))"


def poisson(nx=4, n=8):
    """(solver, eigenstrain Expression, callable eigenstress, boundary data, the eigenstrain as a callable) of a PoissonHMM with a
    TwoPhase coefficient."""
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: 0.02 * (1.0 + 4.0 * x[0]), lambda x: 0.1 + 0.05 * x[1])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), tp, lambda x: 1.0 + x[0], mesh.create_unit_square(n, n), 0.01)
    E = Expression([f"{ALPHA}*f[0]", f"0.5*{ALPHA}*f[0] + 0.002*p[0]*y[1]"], p=[1.5], fields=("dT",))
    Ec = lambda x, y: [_alpha(y) * dT(x), 0.5 * _alpha(y) * dT(x) + 0.002 * 1.5 * y[1]]
    P = lambda x, y: [-(tp(x, y) * e) for e in Ec(x, y)]
    return h, E, P, lambda X: 0.3 * X[0] * X[1], Ec


def elasticity(nx=2, n=6):
    """The same for a LinearElasticityStratifiedHMM in 2D: an isotropic thermal strain and a small shear, the shear DOUBLED in E."""
    lam_in, mu_in = (lambda x: 2.0 + 0.5 * x[0]), (lambda x: 1.5 + 0.25 * x[1])
    lam_out, mu_out = (lambda x: 0.6 + 0.2 * x[1]), (lambda x: 0.4 + 0.1 * x[0])
    tp = hmm.TwoPhase(lambda y: W.wrapped_disc(y[0], y[1]), lambda x: hmm.Lame(lam_in(x), mu_in(x)), lambda x: hmm.Lame(lam_out(x), mu_out(x)))
    h = hmm.LinearElasticityStratifiedHMM(mesh.create_unit_square(nx, nx), tp, lambda x: np.array([0.0, -1.0]), mesh.create_unit_square(n, n), 0.01,
                                          lambda x: np.array([[1.0, 0.1], [0.2, 0.9]]))
    E = Expression([f"{ALPHA}*f[0]", f"0.75*{ALPHA}*f[0]", "0.004*f[0]*y[1]"], fields=("dT",))  # e00, e11, 2 e01

    Ec = lambda x, y: [_alpha(y) * dT(x), 0.75 * _alpha(y) * dT(x), 0.004 * dT(x) * y[1]]

    def P(x, y):
        A = tp(x, y)
        e00, e11, g01 = Ec(x, y)
        tr = e00 + e11
        return [-(A.lam * tr + 2.0 * A.mu * e00), -(A.lam * tr + 2.0 * A.mu * e11), -(A.mu * g01)]

    return h, E, P, lambda X: np.stack([0.1 * X[1] ** 2, 0.2 * X[0]]), Ec


PROBLEMS = {"poisson": poisson, "elasticity": elasticity}


def solve(h, g):
    """solve() with the boundary data g on the whole boundary of the unit square; returns the dof vector."""
    V = h.function_space
    bnd = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1) | np.isclose(x[1], 0) | np.isclose(x[1], 1))
    gf = fem.Function(V)
    gf.interpolate(g)
    h.set_boundary_conditions(fem.dirichletbc(gf, bnd, V))
    return h.solve().x.array.copy()


def fields(h):
    """dT of every macro cell."""
    return dT(h._msh.cell_midpoints().T)


def difference(got, want):
    return np.abs(got - want).max() / np.abs(want).max()
