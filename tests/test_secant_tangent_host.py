"""The consistent tangent of the secant response on the CPU: ``SecantLaw.host_tangent`` -- the NumPy twin the device's
tangent coefficient is held to -- against the analytic formula of tests/secant_tangent_ref.py and against central differences of
``host_values``; the reference's D = A_eff(T) against central differences of the reference's ``mean_flux``; the meaning of the
asymmetry; ``explicit`` and the refusals.  No GPU.
"""

import numpy as np
import pytest

import recon_ref as R
import secant_ref as S
import secant_tangent_ref as TR
from hommx_amd.expr import SecantLaw

KINDS = ["poisson", "poisson_matrix", "elasticity", "elasticity_voigt"]
M2 = np.array([[1.1, 0.2], [-0.1, 0.9]])


def _state(kind, dim, seed, n_el=7, N=2):
    """Seeded strains and positive-definite-looking base / current streams: the formulas under test are pointwise."""
    rng = np.random.default_rng(seed)
    t, n_comp = TR.tensor_size(kind, dim), TR.N_COMP[kind](dim)
    e = rng.standard_normal((N, n_el, t))
    base = 1.0 + rng.random((N, n_el, n_comp))
    cur = 1.0 + rng.random((N, n_el, n_comp))
    return e, cur, base


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_host_tangent_equals_the_analytic_formula(kind, dim):
    """The forward mode and the assembly against dL/de written by hand: agreement to rounding (1e-13 of the largest entry; the two
    sides order their sums differently), the asymmetry of a potential law at most 1e-14."""
    law, dlaw = TR.potential_law(kind, dim)
    e, cur, base = _state(kind, dim, 100 + dim)
    T, asym = law.host_tangent(e, cur, base, np.zeros((len(e), 3)))
    for c in range(len(e)):
        ref = TR.element_tangent(kind, dim, e[c], cur[c], base[c], dlaw)
        assert np.abs(ref - ref.transpose(0, 2, 1)).max() <= 1e-14 * np.abs(ref).max()
        assert np.abs(T[c] - 0.5 * (ref + ref.transpose(0, 2, 1))).max() <= 1e-13 * np.abs(ref).max()
    print(kind, dim, "asymmetry", asym)
    assert np.all(asym <= 1e-14)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_host_tangent_equals_central_differences_of_host_values(kind, dim):
    """T = d(material(L(e)) e)/de at cur = L(e): the flux of the law's own coefficient, differenced in e (h = 1e-6: 1e-8 of the
    largest entry covers the h^2 truncation and eps / h rounding)."""
    law, _ = TR.potential_law(kind, dim)
    e, _, base = _state(kind, dim, 200 + dim)
    x = np.zeros((len(e), 3))
    t = e.shape[2]
    material = lambda c: np.stack([TR.material(kind, dim, c[k]) for k in range(len(c))])
    flux = lambda ee: np.einsum("cemn,cen->cem", material(law.host_values(ee, np.zeros_like(ee), base, x)), ee)
    cur = law.host_values(e, np.zeros_like(e), base, x)
    T, _ = law.host_tangent(e, cur, base, x)
    h, F = 1e-6, np.zeros_like(T)
    for n in range(t):
        d = np.zeros(t)
        d[n] = h
        F[..., n] = (flux(e + d) - flux(e - d)) / (2 * h)
    err = np.abs(T - F).max() / np.abs(T).max()
    print(kind, dim, f"|T - FD| = {err:.2e}")
    assert err <= 1e-8


def test_the_seed_rows_leave_the_existing_passes_alone():
    """``_run`` picks its seeds by a rule; the default rule is the one of the expression passes."""
    from hommx_amd.expr import Expression

    ex = Expression("p[0]*x[0] + f[0]**2", p=[2.0], fields=1)
    yq, w = np.zeros((3, 1, 2)), np.ones(1)
    d = ex.host_tangents(np.array([[0.5, 0.0, 0.0, 3.0]]), yq, w)
    assert np.array_equal(d[0, :, 0], [0.5, 6.0])


CELLS = [("poisson", 2, 8, np.array([0.8, -0.5])), ("elasticity", 2, 5, np.array([0.5, -0.3, 0.4]))]


def _base(kind, dim, n, seed=1):
    rng = np.random.default_rng(seed)
    n_el = (2 if dim == 2 else 6) * n ** dim
    if kind == "poisson":
        return 1.0 + 9.0 * (rng.random(n_el) < 0.3)
    return np.stack([1.0 + rng.random(n_el), 2.0 + 3.0 * (rng.random(n_el) < 0.4)], axis=-1)


def _fd(kind, dim, n, law, base, xi, M, h=1e-5):
    t = len(xi)
    F = np.zeros((t, t))
    solve = S.solver(kind, dim, n)
    for j in range(t):
        d = np.zeros(t)
        d[j] = h
        fp = S.iterate(solve, law, base, xi + d, M=M, max_iter=200, tol=1e-14)["mean_flux"]
        fm = S.iterate(solve, law, base, xi - d, M=M, max_iter=200, tol=1e-14)["mean_flux"]
        F[:, j] = (fp - fm) / (2 * h)
    return F


@pytest.mark.parametrize("with_M", [0, 1])
@pytest.mark.parametrize("kind,dim,n,xi", CELLS, ids=["p2", "e2"])
def test_reference_tangent_equals_central_differences_of_mean_flux(kind, dim, n, xi, with_M):
    """D = A_eff of the linear cell problem with coefficient T_K is d mean_flux / d xi: 1e-8 of max |D| (h = 1e-5, tol = 1e-14; about
    2e-11 observed), and it is NOT the secant tensor."""
    law, dlaw = TR.potential_law(kind, dim)
    base, M = _base(kind, dim, n), (M2 if with_M else None)
    r = TR.tangent(kind, dim, law, dlaw, base, xi, M, n=n, max_iter=200, tol=1e-14)
    assert r["status"] == 0 and r["rounds"] < 200 and r["asymmetry"] <= 1e-14
    F = _fd(kind, dim, n, law, base, xi, M)
    err = np.abs(r["D"] - F).max() / np.abs(r["D"]).max()
    apart = np.abs(r["D"] - r["A"]).max() / np.abs(r["D"]).max()
    print(kind, "M" if with_M else "-", f"rounds {r['rounds']}  |D - FD| = {err:.2e} of max |D|; D against the secant tensor: {apart:.2f}")
    assert err <= 1e-8
    assert apart > 0.05


def test_the_asymmetry_carries_meaning():
    """The mu law without a potential: the element tangents are not symmetric (above 1e-3), and the tangent of the symmetrised law is
    off the true derivative by more than 1e-4 -- a quasi-Newton tangent, which the number announces."""
    kind, dim, n, xi = CELLS[1]
    law, dlaw = TR.potential_law(kind, dim, asymmetric=True)
    base = _base(kind, dim, n)
    r = TR.tangent(kind, dim, law, dlaw, base, xi, None, n=n, max_iter=200, tol=1e-14)
    assert r["status"] == 0
    err = np.abs(r["D"] - _fd(kind, dim, n, law, base, xi, None)).max() / np.abs(r["D"]).max()
    cur = np.asarray(r["coef"])[None]
    _, asym = law.host_tangent(r["s"][None], cur, base[None], np.zeros((1, 3)))
    print(f"asymmetry {r['asymmetry']:.3e} (twin {asym[0]:.3e}); symmetrised D off the differences by {err:.2e}")
    assert r["asymmetry"] > 1e-3 and err > 1e-4
    assert abs(asym[0] - r["asymmetry"]) <= 1e-12


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_the_potential_laws_converge_on_the_reference(kind, dim):
    """Every potential law of the GPU tests stops with status 0 before max_iter on the reference, with asymmetry at most 1e-14."""
    n = 4 if dim == 2 else 2
    rng = np.random.default_rng(7 + dim)
    n_el = (2 if dim == 2 else 6) * n ** dim
    base = R.random_coef(kind, dim, n_el, rng, contrast=10.0)
    xi = rng.standard_normal(TR.tensor_size(kind, dim))
    law, dlaw = TR.potential_law(kind, dim)
    r = TR.tangent(kind, dim, law, dlaw, base, xi, None, n=n, max_iter=60, tol=1e-12)
    print(kind, dim, "rounds", r["rounds"], "asymmetry", r["asymmetry"])
    assert r["status"] == 0 and r["rounds"] < 60 and r["asymmetry"] <= 1e-14


def test_explicit_and_the_refusals():
    assert SecantLaw("c[0]*(1 + e[0]**2)").explicit
    implicit = SecantLaw("c[0]/(1 + s[1]**2)")
    assert not implicit.explicit
    e = np.zeros((1, 2, 2))
    with pytest.raises(ValueError, match=r"s\[1\]"):
        implicit.host_tangent(e, np.ones((1, 2)), np.ones((1, 2)), np.zeros((1, 3)))
    T, asym = SecantLaw("c[0]").host_tangent(e, 3.0 * np.ones((1, 2)), np.ones((1, 2)), np.zeros((1, 3)))  # the identity law: T = material
    assert np.array_equal(T[0, 0], 3.0 * np.eye(2)) and asym[0] == 0.0


def _plan_shaped(kind, dim=2, n_micro=8, n_el=128, n_nodes=64, device=0):
    """What ``MicroCellPlan._check_tangent`` reads of a plan, without a device: the checks run before anything touches the library."""
    from hommx_amd.batch import MicroCellPlan

    p = MicroCellPlan.__new__(MicroCellPlan)
    p._h = None
    p.kind, p.dim, p.n_micro, p.n_el, p.n_nodes, p.device = kind, dim, n_micro, n_el, n_nodes, device
    return p


@pytest.mark.parametrize("entry", ["secant_tangent", "secant_tangent_device"])
def test_the_value_errors_of_both_plan_entries(entry):
    """Both entries refuse, before they read an argument or call the library: an implicit law, naming the s[k] it reads; the plan
    itself, something that is no plan, a sibling of another kind, dim, size or device."""
    def call(p, law, sibling):
        if entry == "secant_tangent":
            return p.secant_tangent(None, None, law, sibling)
        return p.secant_tangent_device(1, None, None, 0, law, sibling, 0, 0, 0, 0, 0)

    explicit = SecantLaw(lam="c[0]", mu="c[1]*(1 + e[2]**2)")
    p, good = _plan_shaped("elasticity"), _plan_shaped("elasticity_voigt")
    assert p.tangent_kind == "elasticity_voigt" and _plan_shaped("elasticity_voigt").tangent_kind == "elasticity_voigt"
    assert _plan_shaped("poisson").tangent_kind == "poisson_matrix" and _plan_shaped("poisson_matrix").tangent_kind == "poisson_matrix"
    for text, k in (("c[1]/(1 + s[0]**2)", 0), ("c[1]/(1 + s[2]**2 + s[1])", 2)):
        with pytest.raises(ValueError, match=rf"the law reads s\[{k}\]: the consistent tangent takes an explicit law"):
            call(p, SecantLaw(lam="c[0]", mu=text), good)
    with pytest.raises(ValueError, match="must be another MicroCellPlan, of kind 'elasticity_voigt'"):
        call(p, explicit, p)
    with pytest.raises(ValueError, match="must be another MicroCellPlan"):
        call(p, explicit, None)
    for kind in ("poisson", "poisson_matrix", "elasticity"):
        with pytest.raises(ValueError, match=f"tangent_plan has kind '{kind}'; the tangent kind of a 'elasticity' plan is 'elasticity_voigt'"):
            call(p, explicit, _plan_shaped(kind))
    with pytest.raises(ValueError, match="tangent_plan has kind 'elasticity_voigt'; the tangent kind of a 'poisson' plan is 'poisson_matrix'"):
        call(_plan_shaped("poisson"), SecantLaw("c[0]*e[1]"), good)
    for other in (dict(dim=3), dict(n_micro=9), dict(n_el=130), dict(n_nodes=65), dict(device=1), dict(n_micro=None)):
        with pytest.raises(ValueError, match=r"tangent_plan has \(dim, n_micro, n_el, n_nodes, device\) = "):
            call(p, explicit, _plan_shaped("elasticity_voigt", **other))
    # a sound pair passes the checks: what fails next is the first use of an argument, not a ValueError of the checks
    with pytest.raises(Exception) as err:
        call(p, explicit, good)
    assert "tangent_plan" not in str(err.value) and "explicit law" not in str(err.value)
