"""The reference of the secant iteration beside a load (tests/secant_load_ref.py) on the CPU, before anything leans on it:
a zero load gives ``secant_ref.iterate``; the two laminates of the section against their scalar layer equations; the reference tangent
at the strain the law saw against central differences of the reference's own ``mean_flux``.  No GPU, no library.
"""

import numpy as np
import pytest
from scipy.optimize import brentq

import secant_load_ref as SL
import secant_ref as S
import secant_tangent_ref as TR
from hommx_amd.expr import SecantLaw
from oracle import hommx_oracle as O

M2 = np.array([[1.1, 0.2], [-0.1, 0.9]])
SOFT = "c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"
CELLS = [("poisson", 2, 4, np.array([1.2, -0.7])), ("elasticity", 2, 3, np.array([0.8, -0.5, 0.6]))]


def _base(kind, dim, n, seed=3):
    rng = np.random.default_rng(seed)
    n_el = (2 if dim == 2 else 6) * n**dim
    if kind == "poisson":
        return 1.0 + 3.0 * (rng.random(n_el) < 0.4) + rng.random(n_el)
    return np.stack([1.0 + rng.random(n_el), 2.0 + 3.0 * (rng.random(n_el) < 0.4)], axis=-1)


def _load(kind, dim, n, seed=4):
    rng = np.random.default_rng(seed)
    n_el, t = (2 if dim == 2 else 6) * n**dim, TR.tensor_size(kind, dim)
    return 0.3 * rng.standard_normal((n_el, t)) + 0.2 * rng.standard_normal((1, t))


@pytest.mark.parametrize("eigenstrain", [False, True], ids=["P", "E"])
@pytest.mark.parametrize("with_M", [0, 1])
@pytest.mark.parametrize("kind,dim,n,xi", CELLS, ids=["p2", "e2"])
def test_a_zero_load_is_the_unloaded_reference(kind, dim, n, xi, with_M, eigenstrain):
    """Two assemblies (loads_ref.Cell, recon_ref) of the same rounds: the same stopping round, and 1e-11 of the largest entry on what
    it leaves (the two factorise different orderings of the same matrix)."""
    law, _ = TR.potential_law(kind, dim)
    base, M = _base(kind, dim, n), (M2 if with_M else None)
    want = S.iterate(S.solver(kind, dim, n), law, base, xi, M=M, max_iter=60, tol=1e-10)
    zero = np.zeros((len(base), TR.tensor_size(kind, dim)))
    got = SL.iterate(SL.cells(kind, dim, n), law, base, xi, zero, eigenstrain, M=M, max_iter=60, tol=1e-10)
    assert want["status"] == 0 and got["status"] == 0 and got["rounds"] == want["rounds"]
    for k in ("A", "mean_flux", "coef", "s", "q"):
        dev = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
        print(kind, k, f"{dev:.2e}")
        assert dev <= 1e-11, k


def _laminate(eigenstrain):
    x, cells = O.unit_cell_mesh(2, 8)
    stiff = x[cells].mean(axis=1)[:, 0] < 0.25
    base = np.where(stiff, 10.0, 1.0)
    load = np.stack([np.where(stiff, 0.5, -0.2), np.zeros(len(base))], axis=-1)
    return SL.iterate(SL.cells("poisson", 2, 8), SecantLaw(SOFT), base, np.array([2.0, 0.0]), load, eigenstrain, max_iter=60, tol=1e-12)


def layer_value(eigenstrain: bool) -> float:
    """mean_flux[0] of the laminate of DESIGN 4.18 from its scalar layer equations: the normal flux q is constant, and the total
    strains of the layers average to xi_0 = 2.  An eigenstrain: q = b_i a(g_i) g_i, sum theta_i (g_i + E_i) = 2.  A polarisation:
    q = b_i a(e_i) e_i + P_i, sum theta_i e_i = 2."""
    a = lambda s: 0.5 + 0.5 / (1 + s * s)
    b, theta, L = (10.0, 1.0), (0.25, 0.75), (0.5, -0.2)
    if eigenstrain:
        flux = lambda i, e: b[i] * a(e - L[i]) * (e - L[i])
    else:
        flux = lambda i, e: b[i] * a(e) * e + L[i]
    e2_of = lambda e1: (2.0 - theta[0] * e1) / theta[1]
    e1 = brentq(lambda e: flux(0, e) - flux(1, e2_of(e)), -1.0, 3.0, xtol=1e-15, rtol=1e-15)
    return flux(0, e1)


@pytest.mark.parametrize("eigenstrain,rounds,recorded", [(True, 9, 1.4900580114184625), (False, 8, 1.2858069625376947)], ids=["E", "P"])
def test_laminate_against_the_scalar_layer_equations(eigenstrain, rounds, recorded):
    want = layer_value(eigenstrain)
    assert abs(want - recorded) <= 1e-11  # the recorded figure, to the tolerance of its root finder
    r = _laminate(eigenstrain)
    print(f"laminate {'E' if eigenstrain else 'P'}: mean_flux[0] = {r['mean_flux'][0]!r} after {r['rounds']} rounds; layer equations {want!r}")
    assert r["status"] == 0 and r["rounds"] == rounds
    assert abs(r["mean_flux"][0] - want) <= 1e-12
    levin = r["cell"].levin(r["P"][None])[0]  # the effective polarisation of the stopping state, two ways
    assert np.abs(r["mean_flux"] - r["A"] @ np.array([2.0, 0.0]) - levin).max() <= 1e-12


def _fd(make, law, base, xi, load, eigenstrain, M, h=1e-5):
    t = len(xi)
    F = np.zeros((t, t))
    for j in range(t):
        d = np.zeros(t)
        d[j] = h
        fp = SL.iterate(make, law, base, xi + d, load, eigenstrain, M=M, max_iter=200, tol=1e-14)["mean_flux"]
        fm = SL.iterate(make, law, base, xi - d, load, eigenstrain, M=M, max_iter=200, tol=1e-14)["mean_flux"]
        F[:, j] = (fp - fm) / (2 * h)
    return F


@pytest.mark.parametrize("eigenstrain", [False, True], ids=["P", "E"])
@pytest.mark.parametrize("with_M", [0, 1])
@pytest.mark.parametrize("kind,dim,n,xi", CELLS, ids=["p2", "e2"])
def test_reference_tangent_equals_central_differences_of_mean_flux(kind, dim, n, xi, with_M, eigenstrain):
    """D = A_eff of the linear cell problem with the element tangents at the strain the law saw is d mean_flux / d xi beside a load
    too: 1e-8 of max |D| with h = 1e-5 and tol = 1e-14, the step and the bound of the unloaded reference (test_secant_tangent_host.py)."""
    law, dlaw = TR.potential_law(kind, dim)
    base, load, M = _base(kind, dim, n), _load(kind, dim, n), (M2 if with_M else None)
    make = SL.cells(kind, dim, n)
    r = SL.iterate(make, law, base, xi, load, eigenstrain, M=M, max_iter=200, tol=1e-14)
    tan = SL.tangent(kind, dim, dlaw, r, base, xi, M, n=n)
    assert r["status"] == 0 and r["rounds"] < 200 and tan["asymmetry"] <= 1e-14
    F = _fd(make, law, base, xi, load, eigenstrain, M)
    err = np.abs(tan["D"] - F).max() / np.abs(tan["D"]).max()
    print(kind, "M" if with_M else "-", "E" if eigenstrain else "P", f"rounds {r['rounds']}  |D - FD| = {err:.2e} of max |D|")
    assert err <= 1e-8
