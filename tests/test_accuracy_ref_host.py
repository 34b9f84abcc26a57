"""The extended-precision reference of tests/accuracy_ref.py checks itself (CPU only): its two solvers against each other, against a
40-digit mpmath solve, the structured against the mesh path, and the float64 yardsticks of the GPU accuracy tests on every case family
(below 1e-12: an ill-posed input cannot loosen a GPU bound unnoticed).  The derived truth (reconstruction, derivatives, loads): its exact
identities to 1e-16, dA_dM against a central difference of ``truth``, the exact scaling laws under coef 2^k, M 2^j, loads 2^k, and caps on
every yardstick the GPU tests of the derived outputs and of the stratification families use (1e-11; correctors 1e-10).  The truth's second
derivatives d2A: energy form against direct form, symmetry, Euler blocks and concavity on every input the GPU test uses, central second
differences of ``truth``, the scaling laws (also under directions 2^i), and the per-block yardstick under the same cap."""

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


# ------------------------------------------------------------------------------------------------------------------------------
# the derived truth (reconstruction, coefficient and stratification derivatives, loads) and the stratification families
# ------------------------------------------------------------------------------------------------------------------------------

SMALL = [("poisson", 2, 16), ("poisson_matrix", 2, 12), ("elasticity", 2, 10), ("elasticity_voigt", 2, 7),
         ("poisson", 3, 6), ("elasticity", 3, 4), ("poisson_matrix", 3, 3), ("elasticity_voigt", 3, 3)]


def _small_cell(kind, dim, n, m_family="mild"):
    case = ("host", kind, dim, n)
    coef, M, g = R.case_inputs(case, "log2", m_family)
    return case, coef[0], M[0], g, R.derived_inputs(case, coef[0])


def _small(v, ref) -> float:
    return float(np.abs(np.asarray(v, dtype=LD)).max() / np.abs(np.asarray(ref, dtype=LD)).max())


@pytest.mark.parametrize("kind,dim,n", SMALL)
def test_identities_of_the_derived_truth(kind, dim, n):
    """In long double, to 1e-16 of the quantity's largest entry."""
    case, coef, M, g, inp = _small_cell(kind, dim, n)
    ne = len(coef)
    canon = np.transpose(R.voigt_material(kind, coef, dim), (2, 0, 1))  # P^m = V e_m, in long double: lambda + 2 mu is no float64
    T = R.derived_truth(kind, g["x"], g["cells"], g["tp"], coef, M, inp["xi"], np.concatenate([coef[None], inp["directions"][1:]]),
                        inp["weights"], canon, inp["labels"])
    A, xi, W = T["A"], inp["xi"].astype(LD), inp["weights"].astype(LD)
    tol = 1e-16
    assert all(v.dtype == LD for v in T.values() if isinstance(v, np.ndarray))
    assert R.rel(T["mean_strain"], xi) <= tol and R.rel(T["mean_flux"], A @ xi) <= tol and R.rel(T["energy"], xi @ A @ xi) <= tol
    assert R.rel(T["dA"][0], A) <= tol  # Euler: A_H is homogeneous of degree one in the coefficient
    for d in range(3):
        terms = T["grad"] * (coef if d == 0 else inp["directions"][d]).astype(LD)
        assert abs(terms.sum() - (W * T["dA"][d]).sum()) <= tol * np.abs(terms).max(), d
    assert _small(np.einsum("abmn,ab->mn", T["dA_dM"], M.astype(LD)), T["dA_dM"]) <= tol  # the derivative of the invariance under M -> c M
    assert R.rel(T["grad_M"], np.einsum("mn,abmn->ab", W, T["dA_dM"])) <= tol
    assert R.rel(T["P_eff"].T, A) <= tol and R.rel(T["load_energy"], T["C0"] - A) <= tol  # the canonical loads reproduce A_H
    # regions cover the cell
    assert R.rel(T["region_volume"].sum(), 1.0) <= tol and R.rel(T["region_energy"].sum(), T["energy"]) <= tol
    assert R.rel(T["region_volume"] @ T["region_mean_flux"], T["mean_flux"]) <= tol and T["region_max_flux"].max() == T["max_flux"]
    _check_d2A_identities(T, [0], f"{kind} {dim}D n={n}")  # direction 0 is the cell's own coefficient here


TOL_D2A = 1e-15  # the identities of the truth's d2A, of the block's (Euler blocks: the array's) largest entry; measured 2.4e-16 at most


def _check_d2A_identities(T, euler, what):
    """The truth's d2A: the energy form against the direct form per block, symmetry in (a, b) and (m, n), the Euler blocks, and concavity
    (no diagonal block has a positive eigenvalue; the eigenvalues in float64: 1e-16 of the block)."""
    D = T["d2A"]
    scale, eps_ld = np.abs(D).max(), float(np.finfo(LD).eps)
    ident = R.block_rel(T["d2A_direct"], D, euler)
    print(f"{what}: d2A energy form against direct form, per block {ident.max():.1e}")
    assert D.dtype == LD and ident.max() <= TOL_D2A, (what, ident)
    # (the direct form is symmetric in (a, b) only as far as it agrees with the energy form)
    assert float(np.abs(D - np.swapaxes(D, 0, 1)).max() / scale) <= 4 * eps_ld and float(np.abs(D - np.swapaxes(D, 2, 3)).max() / scale) <= 4 * eps_ld
    for k in euler:
        assert float(max(np.abs(D[k]).max(), np.abs(D[:, k]).max()) / scale) <= TOL_D2A, (what, k)
    for a in range(D.shape[0]):
        assert np.linalg.eigvalsh(D[a, a].astype(np.float64)).max() <= TOL_D2A * float(scale), (what, a)


def _central_second_differences(A, coef, dirs, h):
    """d2A[a, b] of the long-double tensor A(coef) by central second differences (the stencils of sens2_ref.central_second_differences).
    ``truth`` reads its coefficient as float64, so every perturbed stream must be one exactly: asserted."""
    nd, A0 = len(dirs), A(coef)

    def at(sa, a, sb=0.0, b=0):
        c = coef.astype(LD) + LD(sa * h) * dirs[a].astype(LD) + LD(sb * h) * dirs[b].astype(LD)
        assert np.array_equal(c.astype(np.float64).astype(LD), c)
        return A(c.astype(np.float64))

    out = np.empty((nd, nd) + A0.shape, dtype=LD)
    for a in range(nd):
        out[a, a] = (at(1, a) - 2 * A0 + at(-1, a)) / LD(h) ** 2
        for b in range(a):
            out[a, b] = out[b, a] = (at(1, a, 1, b) - at(1, a, -1, b) - at(-1, a, 1, b) + at(-1, a, -1, b)) / (4 * LD(h) ** 2)
    return out


FD_STEP = 2.0**-16  # eps_ld^(1/4) = 1.8e-5: truncation h^2 d4A / 12 and rounding 4 eps_ld |A| / h^2 balance (both 2e-10 |A| at d4A ~ |A|)
FD_GRID = 2.0**-20  # coefficient and directions are rounded to this grid, so that coef +- h dir_a +- h dir_b is a float64 exactly


@pytest.mark.parametrize("kind,dim,n,tol", [("poisson", 2, 5, 1e-8), ("elasticity", 3, 3, 1e-6)])
def test_d2A_against_central_second_differences_of_truth(kind, dim, n, tol):
    """The independent check of the truth's d2A: central second differences of ``truth``'s A_H in long double (dense Cholesky: no stopping
    criterion), step 2^-16, with coefficient and directions on a grid of 2^-20 so that no perturbed stream is rounded.  The difference
    quotient's own error is h^2 d4A / 12 + 4 eps_ld |A| / h^2; the directions reach 30 times the smallest coefficient, so d4A is far above |A|.
    Achieved, of the largest entry: 9.2e-10 (Poisson 2D n = 5) and 9.5e-8 (3D elasticity n = 3); ``tol`` is 10 x that."""
    case, coef, M, g, inp = _small_cell(kind, dim, n)
    q = lambda v: np.round(v / FD_GRID) * FD_GRID  # noqa: E731
    coef = q(coef)
    dirs = np.stack([coef, q(inp["directions"][1]), q(inp["directions"][2])])
    T = R.derived_truth(kind, g["x"], g["cells"], g["tp"], coef, M, directions=dirs, solver="dense")
    fd = _central_second_differences(lambda c: R.truth(kind, g["x"], g["cells"], g["tp"], c, M, solver="dense")[0], coef, dirs, FD_STEP)
    err = float(np.abs(fd - T["d2A"]).max() / np.abs(T["d2A"]).max())
    print(f"{kind} {dim}D n={n}: d2A against central second differences of truth {err:.2e}")
    assert err <= tol


@pytest.mark.parametrize("kind,dim,n", [("poisson", 2, 5), ("elasticity_voigt", 2, 4), ("elasticity", 3, 3)])
def test_dA_dM_against_a_central_difference_of_truth(kind, dim, n):
    """Step 2^-20 in long double: truncation h^2 ~ 1e-12, rounding 1e-19 / h ~ 1e-13; agreement to 1e-10."""
    case, coef, M, g, inp = _small_cell(kind, dim, n)
    T = R.derived_truth(kind, g["x"], g["cells"], g["tp"], coef, M)
    h = 2.0**-20
    for a in range(dim):
        for b in range(dim):
            E = np.zeros((dim, dim))
            E[a, b] = h
            Ap = R.truth(kind, g["x"], g["cells"], g["tp"], coef, M + E)[0]
            Am = R.truth(kind, g["x"], g["cells"], g["tp"], coef, M - E)[0]
            assert float(np.abs((Ap - Am) / LD(2 * h) - T["dA_dM"][a, b]).max() / np.abs(T["dA_dM"]).max()) <= 1e-10, (a, b)


@pytest.mark.parametrize("kind,dim,n", [("poisson", 2, 5), ("elasticity", 3, 3)])
def test_scaling_laws_are_exact(kind, dim, n):
    """coef * 2^k, M * 2^j, loads * 2^k with xi, directions and weights fixed: every derived output scales by the power of two of
    accuracy_ref.SCALING_LAWS, to 4 eps_ld of its largest entry, and the argmax stays.  This test decides the laws the GPU sweeps use."""
    case, coef, M, g, inp = _small_cell(kind, dim, n)
    args = (inp["xi"], inp["directions"], inp["weights"])
    T0 = R.derived_truth(kind, g["x"], g["cells"], g["tp"], coef, M, *args, inp["loads"], inp["labels"])
    tol = 4 * float(np.finfo(LD).eps)
    for k, j in ((40, 0), (-40, 0), (0, 20), (0, -20), (0, 10), (40, -20), (-40, 20), (40, 20)):
        T = R.derived_truth(kind, g["x"], g["cells"], g["tp"], coef * 2.0**k, M * 2.0**j, *args, inp["loads"] * 2.0**k, inp["labels"])
        for name, (pk, pj) in R.SCALING_LAWS.items():
            assert R.rel(T[name] * LD(2.0) ** -(k * pk + j * pj), T0[name]) <= tol, (name, k, j)
        assert set(R.SCALING_LAWS) >= set(T) - {"C0", "vol", "s_canon", "norm", "region_norm", "load_norm"}
        assert T["norm"].argmax() == T0["norm"].argmax() and np.array_equal(T["load_norm"].argmax(axis=1), T0["load_norm"].argmax(axis=1))
        assert np.array_equal(T["region_norm"].argmax(axis=1), T0["region_norm"].argmax(axis=1))
    # the third sweep: the directions alone times 2^i.  dA is linear and d2A bilinear in them; nothing else moves
    for i in (20, -20, 7):
        T = R.derived_truth(kind, g["x"], g["cells"], g["tp"], coef, M, inp["xi"], inp["directions"] * 2.0**i, inp["weights"], inp["loads"],
                            inp["labels"])
        for name in set(T) - {"region_norm"}:
            assert R.rel(T[name] * LD(2.0) ** -(i * R.DIRECTION_LAWS.get(name, 0)), T0[name]) <= tol, (name, i)


def test_stratification_families():
    for dim in (2, 3):
        Q = R.stratification_family("rot", dim, 1, 0)[0]
        assert np.allclose(Q @ Q.T, np.eye(dim), atol=1e-15) and np.isclose(np.linalg.det(Q), 1.0) and not np.allclose(Q, np.eye(dim), atol=0.1)
        S = R.stratification_family("squeeze16", dim, 2, 0)
        assert np.allclose(np.linalg.svd(S[0], compute_uv=False), [1.0] * (dim - 1) + [1 / 16]) and np.array_equal(S[0], S[1])
        H = R.stratification_family("shear30", dim, 1, 0)[0]
        assert np.array_equal(H, np.eye(dim) + 30.0 * np.outer(np.eye(dim)[0], np.eye(dim)[dim - 1]))
        assert np.array_equal(R.stratification_family("mild", dim, 2, 5), R.stratification(dim, 2, 5))


CAP = 1e-11  # tensors, fields, derivatives: a condition that keeps a bound from becoming vacuous, not a measurement
CAP_CORRECTORS = 1e-10


@pytest.mark.parametrize("case", R.M_CASES, ids=lambda c: R.case_id(c[1:]))
def test_truth_converges_and_tensor_yardstick_is_capped_on_every_M_family(case):
    """The cases of test_gpu_accuracy.py's stratification tests: ``truth`` converges (a stall above STALL_LIMIT raises) and the float64
    yardsticks of A_H stay below the cap, on log2 and the top-contrast family with shear30, squeeze16 and rot."""
    kind = case[2]
    for family in ("log2", R.top_family(kind)):
        for mf in R.M_CONDITIONING:
            coef, M, g = R.case_inputs(case[1:], family, mf)
            for c in range(R.NC):
                e = R.float64_errors(kind, g["x"], g["cells"], g["tp"], coef[c], M[c], **g["kw"])
                print(f"{R.case_id(case[1:])} {family} {mf} cell {c}: oracle {e['e_oracle']:.1e} cholesky {e['e_cholesky']:.1e} corr {e['e_corr']:.1e}")
                assert e["e_oracle"] <= CAP and e["e_cholesky"] <= CAP and e["e_corr"] <= CAP_CORRECTORS, (family, mf, c, e)


@pytest.mark.parametrize("case", R.DERIVED_CASES, ids=lambda c: R.case_id(R.derived_case(c)[2]))
def test_derived_yardsticks_are_capped(case):
    """Every case, family and cell of test_gpu_accuracy_derived.py: the truth converges and no float64 yardstick passes its cap; d2A per
    block (the largest block of the cell decides), and its truth meets its identities on these very inputs.  The Euler blocks are those
    of cell 0 of the four log2 families, whose coefficient is direction 0: read off the inputs.

    Measured, d2A per block: 4.2e-12 at most (small_wave-elasticity-2-10, log2 shear30, cell 1); below 1e-14 without a hard M."""
    _, _, cs = R.derived_case(case)
    kind = cs[1]
    inp = R.derived_inputs(cs, R.case_inputs(cs, "log2", None)[0][0])
    worst = {}
    for family, mf in R.DERIVED_FAMILIES:
        coef, M, g = R.case_inputs(cs, family or R.top_family(kind), mf)
        for c in range(R.NC):
            a = (kind, g["x"], g["cells"], g["tp"], coef[c], None if M is None else M[c])
            T = R.derived_truth(*a, **inp)
            euler = R.euler_directions(coef[c], inp["directions"])
            assert euler == ([0] if family == "log2" and c == 0 else []), (family, mf, c, euler)
            _check_d2A_identities(T, euler, f"{R.case_id(cs)} {family} {mf} cell {c}")
            e = R.derived_float64_errors(*a, **inp, T=T, **g["kw"])["e"]
            assert e["d2A"].shape == (3, 3)
            print(f"{R.case_id(cs)} {family} {mf} cell {c}: d2A yardstick per block, largest {e['d2A'].max():.1e}")
            for name, v in e.items():
                v = float(np.max(v))
                worst[name] = max(worst.get(name, 0.0), v)
                assert v <= (CAP_CORRECTORS if name in R.CORRECTOR_QUANTITIES else CAP), (family, mf, c, name, v)
    print(R.case_id(cs), {k: f"{v:.1e}" for k, v in worst.items()})
