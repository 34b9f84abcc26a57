"""The extended-precision reference of tests/accuracy_ref.py checks itself (CPU only): its two solvers against each other, against a
40-digit mpmath solve, the structured against the mesh path, and the float64 yardsticks of the GPU accuracy tests on every case family
(below 1e-12: an ill-posed input cannot loosen a GPU bound unnoticed)."""

import numpy as np
import pytest

import accuracy_ref as R

LD = R.LD


def _families(kind):
    return [(f, m) for f in R.FAMILIES[kind] for m in (False, True)]


@pytest.mark.parametrize("kind,dim,n", [("poisson", 2, 16), ("poisson_matrix", 2, 12), ("elasticity", 2, 10), ("elasticity_voigt", 2, 7),
                                        ("poisson", 3, 6), ("elasticity", 3, 4), ("poisson_matrix", 3, 3), ("elasticity_voigt", 3, 3)])
def test_dense_and_refined_solvers_agree(kind, dim, n):
    """All four kinds, with and without M, every family: tensors and correctors agree to 1e-17."""
    x, cells, tp = R.structured(dim, n)
    for family, with_M in _families(kind):
        coef, M = R.structured_inputs(kind, dim, n, family, with_M)
        A1, c1 = R.truth(kind, x, cells, tp, coef[0], None if M is None else M[0], solver="dense")
        A2, c2 = R.truth(kind, x, cells, tp, coef[0], None if M is None else M[0], solver="refine")
        assert A1.dtype == LD and c1.dtype == LD
        assert R.rel(A1, A2) < 1e-17, (family, with_M)
        assert R.rel(c1, c2) < 1e-17, (family, with_M)
        assert float(np.abs(A2 - A2.T).max()) <= 1e-18 * float(np.abs(A2).max())


def _mpmath_poisson(x, cells, tp, coef, M):
    """Scalar Poisson cell problem in 40-digit arithmetic, written out element by element (no NumPy arithmetic): energy-form tensor."""
    import mpmath as mp

    mp.mp.dps = 40
    dim = cells.shape[1] - 1
    nn = int(tp.max()) + 1
    Mm = mp.matrix([[mp.mpf(float(M[i, j])) for j in range(dim)] for i in range(dim)])
    K = mp.zeros(nn, nn)
    B = mp.zeros(nn, dim)
    els = []
    for e, cell in enumerate(cells):
        P = mp.matrix([[mp.mpf(1)] + [mp.mpf(float(x[v, i])) for i in range(dim)] for v in cell])
        G = mp.inverse(P)  # column a: coefficients of the P1 basis function a; rows 1.. are its gradient
        g = [Mm * mp.matrix([G[1 + i, a] for i in range(dim)]) for a in range(dim + 1)]
        vol = abs(mp.det(P)) / (2 if dim == 2 else 6)
        a_e = mp.mpf(float(coef[e]))
        els.append((vol, a_e, g, [int(tp[v]) for v in cell]))
        for a in range(dim + 1):
            for b in range(dim + 1):
                K[int(tp[cell[a]]), int(tp[cell[b]])] += vol * a_e * (g[a].T * g[b])[0]
            for m in range(dim):
                B[int(tp[cell[a]]), m] -= vol * a_e * g[a][m]
    chi = mp.zeros(nn, dim)
    for m in range(dim):
        sol = mp.lu_solve(K[1:, 1:], B[1:, m])
        for i in range(1, nn):
            chi[i, m] = sol[i - 1]
    A = mp.zeros(dim, dim)
    for vol, a_e, g, nodes in els:
        F = []
        for m in range(dim):
            f = mp.matrix([mp.mpf(1) if i == m else mp.mpf(0) for i in range(dim)])
            for a in range(dim + 1):
                f += chi[nodes[a], m] * g[a]
            F.append(f)
        for m in range(dim):
            for k in range(dim):
                A[m, k] += vol * a_e * (F[m].T * F[k])[0]
    return A, chi


@pytest.mark.parametrize("dim", [2, 3])
def test_against_40_digit_mpmath(dim):
    """n = 3, contrast 1e4, with M: tensor and correctors against mpmath at 40 digits, compared in mpmath (no rounding to float64)."""
    import mpmath as mp

    x, cells, tp = R.structured(dim, 3)
    coef, M = R.structured_inputs("poisson", dim, 3, "tp4", True)
    A, chi = R.truth("poisson", x, cells, tp, coef[0], M[0])
    Am, chim = _mpmath_poisson(x, cells, tp, coef[0], M[0])
    ld = lambda v: mp.mpf(str(np.format_float_scientific(v, precision=24, unique=False)))  # noqa: E731  a long double is exact in 21 digits + margin
    scale = max(abs(Am[i, j]) for i in range(dim) for j in range(dim))
    assert max(abs(ld(A[i, j]) - Am[i, j]) for i in range(dim) for j in range(dim)) < mp.mpf("1e-18") * scale
    nn = chi.shape[0]
    mean = [sum(chim[i, m] for i in range(nn)) / nn for m in range(dim)]
    cs = max(abs(chim[i, m] - mean[m]) for i in range(nn) for m in range(dim))
    assert max(abs(ld(chi[i, m]) - (chim[i, m] - mean[m])) for i in range(nn) for m in range(dim)) < mp.mpf("1e-17") * cs


@pytest.mark.parametrize("dim,n,kind", [(2, 6, "poisson_matrix"), (2, 5, "elasticity"), (3, 3, "poisson"), (3, 3, "elasticity_voigt")])
def test_structured_and_mesh_paths_agree(dim, n, kind):
    """create_unit_square / create_unit_cube through the mesh path (the package's periodic constraint) against the oracle's structured
    tables: the same cell, so the same numbers to long-double rounding (the node numbering differs, the element order does not)."""
    from hommx_amd import mesh as Mm

    msh = Mm.create_unit_square(n, n) if dim == 2 else Mm.create_unit_cube(n, n, n)
    xm, cm, tpm = R.mesh_arrays(msh)
    x, cells, tp = R.structured(dim, n)
    assert cm.shape == cells.shape
    coef, M = R.structured_inputs(kind, dim, n, "log2", True)
    A1, c1 = R.truth(kind, x, cells, tp, coef[0], M[0])
    A2, c2 = R.truth(kind, xm, cm, tpm, coef[0], M[0])
    assert R.rel(A2, A1) < 1e-17
    bs = c1.shape[0] // (int(tp.max()) + 1)
    # the correctors as fields on the mesh vertices
    f1 = c1.reshape(-1, bs, c1.shape[1])[tp]
    f2 = c2.reshape(-1, bs, c2.shape[1])[tpm]
    if np.allclose(xm, x):
        assert R.rel(f2, f1) < 1e-17


def _yardstick_cases():
    seen = []
    for group in R.STRUCTURED_CASES.values():
        for _, kind, dim, n, _ in group:
            if (kind, dim, n) not in seen:
                seen.append((kind, dim, n))
    return seen


@pytest.mark.parametrize("kind,dim,n", _yardstick_cases())
def test_yardstick_stays_below_1e12_structured(kind, dim, n):
    x, cells, tp = R.structured(dim, n)
    for family, with_M in _families(kind):
        coef, M = R.structured_inputs(kind, dim, n, family, with_M)
        for c in range(R.NC):
            e = R.float64_errors(kind, x, cells, tp, coef[c], None if M is None else M[c], n=n)
            assert e["e_oracle"] < 1e-12 and e["e_cholesky"] < 1e-12, (family, with_M, c, e)
            assert R.FACTOR * R.FLOOR_EPS * R.EPS <= e["bound"] < 32e-12


@pytest.mark.parametrize("case", R.MESH_CASES[:2], ids=lambda c: c[2])
def test_yardstick_stays_below_1e12_mesh(case):
    _, kind, builder, args, _ = case
    for family, with_M in _families(kind):
        msh, coef, M = R.mesh_inputs(kind, builder, args, family, with_M)
        x, cells, tp = R.mesh_arrays(msh)
        for c in range(R.NC):
            e = R.float64_errors(kind, x, cells, tp, coef[c], None if M is None else M[c], msh=msh)
            assert e["e_oracle"] < 1e-12 and e["e_cholesky"] < 1e-12, (family, with_M, c, e)


def test_truth_scales_exactly_with_a_power_of_two():
    """What the magnitude sweep relies on: scaling the coefficient by 2^k scales every long-double intermediate exactly."""
    x, cells, tp = R.structured(2, 8)
    coef, M = R.structured_inputs("poisson", 2, 8, "log2", True)
    A0, c0 = R.truth("poisson", x, cells, tp, coef[0], M[0])
    for k in (-40, 40):
        A, c = R.truth("poisson", x, cells, tp, coef[0] * 2.0**k, M[0])
        assert R.rel(A * LD(2.0) ** -k, A0) < 1e-18 and R.rel(c, c0) < 1e-17
