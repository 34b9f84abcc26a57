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

Stratification: one case per kernel family, the padded fused blocks and both mesh routes (accuracy_ref.M_CASES) with M far from the
identity (shear 30, a squeeze by 16 under a rotation, a pure rotation) under the same rule, and with M 2^j, coef 2^k, where A_H 2^-k must
return the numbers of (k, j) = (0, 0) to 16 eps: both normalisations take an exponent from M.
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


def _m_reference(case, family, mf, c):
    coef, M, g = R.case_inputs(case, family, mf)
    return _reference(("M", R.case_id(case), family, mf, c), case[1], g["x"], g["cells"], g["tp"], coef[c], M[c], **g["kw"])


@pytest.mark.parametrize("case", R.M_CASES, ids=lambda c: R.case_id(c[1:]))
def test_stratification_conditioning(results, case):
    """M far from the identity -- shear 30, a squeeze by 16 under a rotation, a pure rotation -- on log2 and the kind's top-contrast family,
    one case per kernel family and the padded fused blocks: the rule of every other test here, with the truth and the yardsticks of that
    very (coef, M).  tests/test_accuracy_ref_host.py holds those yardsticks below 1e-11; accuracy_ref.SOFTENED lists the softened cases."""
    res, case = results(case[0]), case[1:]
    cid = R.case_id(case)
    for family in ("log2", R.top_family(case[1])):
        for mf in R.M_CONDITIONING:
            A, info = res[f"MA|{cid}|{family}|{mf}"], res[f"Minfo|{cid}|{family}|{mf}"]
            for c in range(R.NC):
                T, e = _m_reference(case, family, mf, c)
                _check(A[c], info[c], T, e, f"{cid} {family} {mf} cell {c}")


@pytest.mark.parametrize("case", R.M_CASES, ids=lambda c: R.case_id(c[1:]))
def test_stratification_scale(results, case):
    """log2 with M = (I + 0.3 N) 2^j and coef 2^k: A_H 2^-k is invariant under the scale of M (exactly so in long double:
    tests/test_accuracy_ref_host.py), so every (k, j) meets the bound of the (0, 0) truth with info 0, and -- a power of two commutes with
    every rounding -- returns the (0, 0) numbers of the device again, to 16 eps of the largest entry.  This is what pins the exponent that
    both normalisations take from M (k_poisson2d_fused, k_coef_normalise)."""
    res, case = results(case[0]), case[1:]
    cid = R.case_id(case)
    base = res[f"MsA|{cid}|0|0"]
    failures = []
    for c in range(R.NC):
        T, e = _m_reference(case, "log2", "mild", c)
        for k, j in R.M_SCALES:
            A, info = res[f"MsA|{cid}|{k}|{j}"][c] * 2.0**-k, res[f"Msinfo|{cid}|{k}|{j}"][c]
            err, d = R.rel(A, T[0]), float(np.abs(A - base[c]).max() / np.abs(base[c]).max())
            print(f"M scale {cid} cell {c} coef 2^{k} M 2^{j}: e = {err:.2e} bound {e['bound']:.1e} ratio {err / (e['bound'] / R.FACTOR):.2f}"
                  f"  against (0, 0): {d:.2e}  info {info}")
            if info != 0 or not err <= e["bound"] or not d <= 16 * R.EPS:
                failures.append((k, j, c, err, d, int(info)))
    assert not failures, (cid, failures)
