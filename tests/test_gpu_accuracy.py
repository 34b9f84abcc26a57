"""Accuracy of every elimination route against extended precision, on an MI355X (-m gpu).

For every cell   e = max|A_gpu - T| / max|T|  <=  32 * max(e_oracle_schur, e_cholesky_schur, 16 eps),   T = accuracy_ref.truth (long double),
the two float64 yardsticks from accuracy_ref.float64_errors on the same inputs: the kernels evaluate the same Schur form, whose error is
the C0 - G cancellation plus elimination roundoff; 2^5 covers another summation order and the explicit block inverses.  Correctors: the
same rule with the oracle's mean-free correctors as the yardstick.  No bound here is computed from a GPU result.

Every case runs two seeded cells per coefficient family (log-uniform 1e2; two-phase 1e4 and 1e7 for Poisson, 1e5 in both Lame parameters
for elasticity), with and without M = I + 0.3 N, and the route is asserted through plan.kernel (tests/accuracy_gpu.py).  Environment
knobs are read when a plan is created, so the forced routes (staged tree, plane elimination) run in one fresh child process each.

Magnitude sweep: one mild case per kernel family with the coefficient scaled by 2^k, k in {-40, -20, 0, 20, 30, 40} (k = 30 .. 37 is an
elastic modulus in pascals).  The truth scales exactly; the same bound holds at every k and info stays 0.
"""

import numpy as np
import pytest

import accuracy_gpu as G
import accuracy_ref as R

pytestmark = pytest.mark.gpu

_truth_cache = {}


def _reference(key, kind, x, cells, tp, coef, M, **kw):
    """(truth, yardstick errors) of one cell, computed once and shared between the groups that run the same inputs."""
    if key not in _truth_cache:
        T = R.truth(kind, x, cells, tp, coef, M)
        _truth_cache[key] = (T, R.float64_errors(kind, x, cells, tp, coef, M, T=T, **kw))
    return _truth_cache[key]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cache = {}

    def get(group):
        if group not in cache:
            cache[group] = G.run_accuracy_group(group) if group == "default" else G.run_in_child("accuracy", group, tmp_path_factory.mktemp(group))
        return cache[group]

    return get


def _check(A, info, T, e, what):
    assert np.all(info == 0), (what, info)
    err = R.rel(A, T[0])
    print(f"{what}: e = {err:.2e}  oracle {e['e_oracle']:.1e}  cholesky {e['e_cholesky']:.1e}  bound {e['bound']:.1e}  ratio {err / (e['bound'] / R.FACTOR):.2f}")
    assert err <= e["bound"], (what, err, e)


def _structured_ids():
    return [(g,) + c for g, cs in R.STRUCTURED_CASES.items() for c in cs]


@pytest.mark.parametrize("group,kernel,kind,dim,n,flags", _structured_ids(), ids=lambda v: str(v))
def test_structured_routes(results, group, kernel, kind, dim, n, flags):
    res = results(group)
    x, cells, tp = R.structured(dim, n)
    for family in R.FAMILIES[kind]:
        for with_M in (False, True):
            coef, M = R.structured_inputs(kind, dim, n, family, with_M)
            A = res[f"A|{G.skey(kind, dim, n, flags)}|{family}|{int(with_M)}"]
            info = res[f"info|{G.skey(kind, dim, n, flags)}|{family}|{int(with_M)}"]
            for c in range(R.NC):
                Mc = None if M is None else M[c]
                T, e = _reference((kind, dim, n, family, with_M, c), kind, x, cells, tp, coef[c], Mc, n=n)
                _check(A[c], info[c], T, e, f"{group} {kernel} {kind} {dim}D n={n} {family} M={int(with_M)} cell {c}")


@pytest.mark.parametrize("case", R.MESH_CASES, ids=lambda c: f"{c[0]}-{c[2]}")
def test_mesh_routes(results, case):
    kernel, kind, builder, args, route = case
    res = results("default")
    for family in R.FAMILIES[kind]:
        for with_M in (False, True):
            msh, coef, M = R.mesh_inputs(kind, builder, args, family, with_M)
            x, cells, tp = R.mesh_arrays(msh)
            A = res[f"A|{G.mkey(kind, builder, args, route)}|{family}|{int(with_M)}"]
            info = res[f"info|{G.mkey(kind, builder, args, route)}|{family}|{int(with_M)}"]
            for c in range(R.NC):
                Mc = None if M is None else M[c]
                T, e = _reference((kind, builder, args, family, with_M, c), kind, x, cells, tp, coef[c], Mc, msh=msh)
                _check(A[c], info[c], T, e, f"{kernel} {kind} {builder}{args} {family} M={int(with_M)} cell {c}")


@pytest.mark.parametrize("ckernel,kind,dim,n,group", R.CORRECTOR_CASES, ids=lambda v: str(v))
def test_correctors(results, ckernel, kind, dim, n, group):
    """The three corrector paths: substitution on the fused kernel's stored block inverses, the plane elimination behind a small-block plan,
    the tree's back substitution.  Mean-free correctors[t, n_dof] against the truth; the tensor of the same call against its own bound."""
    res = results(group)
    x, cells, tp = R.structured(dim, n)
    for family in R.FAMILIES[kind]:
        for with_M in (False, True):
            coef, M = R.structured_inputs(kind, dim, n, family, with_M)
            tail = f"{G.skey(kind, dim, n, 0)}|{family}|{int(with_M)}"
            A, chi, info = res["corrA|" + tail], res["corr|" + tail], res["corrinfo|" + tail]
            for c in range(R.NC):
                Mc = None if M is None else M[c]
                T, e = _reference((kind, dim, n, family, with_M, c), kind, x, cells, tp, coef[c], Mc, n=n)
                what = f"correctors {ckernel} {kind} {dim}D n={n} {family} M={int(with_M)} cell {c}"
                _check(A[c], info[c], T, e, what)
                err = R.rel(chi[c].T, T[1])
                print(f"{what}: e_corr = {err:.2e}  oracle {e['e_corr']:.1e}  bound {e['bound_corr']:.1e}")
                assert err <= e["bound_corr"], (what, err, e)


def _sweep_ids():
    return list(R.SWEEP_CASES) + [("default",) + R.SWEEP_MESH]


@pytest.mark.parametrize("case", _sweep_ids(), ids=lambda c: f"{c[1]}-{c[2]}-{c[3]}-{c[4]}")
def test_magnitude_sweep(results, case):
    """coef * 2^k: the truth scales exactly (tests/test_accuracy_ref_host.py), so it is computed once; same bound at every k, info stays 0."""
    group = case[0]
    res = results(group)
    if isinstance(case[3], str):  # mesh case
        _, kernel, kind, builder, args, route = case
        msh, coef, M = R.mesh_inputs(kind, builder, args, "log2", True)
        x, cells, tp = R.mesh_arrays(msh)
        key, kw, ck = G.mkey(kind, builder, args, route), {"msh": msh}, (kind, builder, args, "log2", True)
    else:
        _, kernel, kind, dim, n, flags = case
        coef, M = R.structured_inputs(kind, dim, n, "log2", True)
        x, cells, tp = R.structured(dim, n)
        key, kw, ck = G.skey(kind, dim, n, flags), {"n": n}, (kind, dim, n, "log2", True)
    failures = []
    for c in range(R.NC):
        T, e = _reference(ck + (c,), kind, x, cells, tp, coef[c], M[c], **kw)
        for k in R.SWEEP_K:
            A, info = res[f"sweepA|{key}|{k}"][c], res[f"sweepinfo|{key}|{k}"][c]
            err = R.rel(A * 2.0**-k, T[0])
            print(f"sweep {kernel} {key} cell {c} 2^{k}: e = {err:.2e} bound {e['bound']:.1e} info {info}")
            if info != 0 or not err <= e["bound"]:
                failures.append((k, c, err, int(info)))
    assert not failures, (kernel, key, failures)


@pytest.mark.parametrize("kind,dim,n", R.SWEEP_LOAD_CASES, ids=lambda v: str(v))
def test_magnitude_sweep_correctors_and_loads(results, kind, dim, n):
    """Correctors and user-supplied polarisation loads at 2^-40, 1, 2^40, coefficient and loads scaled together.

    The canonical correctors do not depend on the scale: against the truth, with the corrector bound, at every k.  The load outputs scale
    exactly -- P_eff, energy and the mean flux by 2^k, the load correctors not at all -- and a scaling by a power of two commutes with every
    rounding, so a route whose arithmetic does not depend on the magnitude returns the k = 0 numbers again: 16 eps of the largest entry is
    allowed (the precision of the format, not a measured figure).  This is what pins the scaling of the load rows next to the
    normalised stiffness (blocked.hip, multifrontal.hip)."""
    res = results("default")
    x, cells, tp = R.structured(dim, n)
    coef, M = R.structured_inputs(kind, dim, n, "log2", True)
    key = G.skey(kind, dim, n, 0)
    tol = 16 * R.EPS
    for k in R.SWEEP_LOAD_K:
        assert np.all(res[f"lsw_info|{key}|{k}"] == 0), k
        chi = res[f"lsw_chi|{key}|{k}"]
        for c in range(R.NC):
            T, e = _reference((kind, dim, n, "log2", True, c), kind, x, cells, tp, coef[c], M[c], n=n)
            err = R.rel(chi[c].T, T[1])
            print(f"sweep correctors {key} cell {c} 2^{k}: e_corr = {err:.2e} bound {e['bound_corr']:.1e}")
            assert err <= e["bound_corr"], (k, c, err, e)
        for name, power in (("Peff", 1), ("energy", 1), ("mean", 1), ("lchi", 0)):
            got, ref = res[f"lsw_{name}|{key}|{k}"] * 2.0 ** (-k * power), res[f"lsw_{name}|{key}|0"]
            d = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"sweep loads {key} {name} 2^{k}: {d:.2e}")
            assert d <= tol, (name, k, d)
