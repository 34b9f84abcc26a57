"""The load solve of the fused 2D family by substitution on the extended factor record, host side: the passes
k_fused2d_subst_rhs implements, stated in NumPy (tests/fused_rhs_ref.py), against a dense solve for loads of loads_ref; the canonical
loads against fused_subst_ref; the same passes with the device's signs, couplings and magnitude exponent; the accessor that names a
plan's load route (CPU only).

Bound: 1e-11 relative to the largest corrector entry, the bar tests/test_loads_host.py holds its reference to."""

import ctypes
import functools
import os

import numpy as np
import pytest

import fused_rhs_ref as R
import fused_subst_ref as F
import loads_ref as L

SIZES = [3, 4, 5, 16, 17, 20]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from hommx_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _cell(n, with_M):
    """A cell of contrast 1e2, its dense K, two random loads, their load vectors and the dense pinned solve (mean-free); read only."""
    rng = np.random.default_rng(100 * n + with_M)
    coef = L.random_coef("poisson", 2, 2 * n * n, rng)
    M = L.random_M(2, rng) if with_M else None
    cell = L.structured("poisson", 2, n, coef, M)
    P = L.random_loads(rng, 2, cell.n_el, 2)
    f = cell.load_vector(P).T  # [n n, loads]
    K = R.dense_stiffness(cell)
    chi = np.zeros_like(f)
    chi[:-1] = np.linalg.solve(K[:-1, :-1], -f[:-1])
    chi -= chi.mean(axis=0, keepdims=True)
    return cell, K, P, f, chi


def _err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_passes_reproduce_a_dense_solve(n, with_M):
    """A - D on the extended record for loads that are no canonical ones: every sign, the Horner pass (one step at n = 3), N_last."""
    cell, K, _, f, chi = _cell(n, with_M)
    assert np.abs(f.sum(axis=0)).max() < 1e-12 * np.abs(f).max()  # compatible
    got = R.correctors(R.factor(K, n), f, n)
    err = _err(got, chi)
    print(n, with_M, err)
    assert err < 1e-11


@pytest.mark.parametrize("n", SIZES)
def test_dense_solve_is_the_reference_of_the_gpu_tests(n):
    """The dense solve above and loads_ref.Cell.solve (sparse LU, what tests/test_gpu_fused_loads.py compares with) are the same thing."""
    cell, _, P, f, chi = _cell(n, True)
    want = cell.solve(P)
    assert np.array_equal(want["f"].T, f)
    assert _err(chi, want["chi"].T) < 1e-11


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_canonical_loads_reproduce_the_canonical_substitution(n, with_M):
    """P = material(coef) e_m: the general passes give what fused_subst_ref.correctors gives from the record of the elimination itself."""
    cell, K, _, _, _ = _cell(n, with_M)
    f = cell.load_vector(np.transpose(cell.V, (2, 0, 1))).T
    want = F.correctors(K, -f, n)
    assert _err(R.correctors(R.factor(K, n), f, n), want) < 1e-11
    assert _err(want, cell.chi_canon.T) < 1e-11


@pytest.mark.parametrize("esh", [0, 7, -40])
@pytest.mark.parametrize("n", SIZES)
def test_device_form_reproduces_a_dense_solve(n, esh):
    """N' = -S^-1, y = -x, couplings as two vectors (the header's is C^T), the record of the coefficient scaled by 2^-esh and the load scaled
    with it: the kernel's statement line by line.  A lost esh is off by the factor 2^esh."""
    _, K, _, f, chi = _cell(n, True)
    d = R.device_record(K, n, esh)
    assert _err(R.device_correctors(d, f, n), chi) < 1e-11
    if esh:
        assert _err(R.device_correctors(dict(d, esh=0), f, n), chi) > 0.5


def test_library_exports_load_kernel_name(lib):
    from hommx_amd import _lib

    assert "hommx_plan_load_kernel_name" in _lib.EXPORTED_SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "hommx_plan_load_kernel_name")


def test_load_kernel_name_of_a_null_plan(lib):
    """As hommx_plan_corrector_kernel_name: the empty string."""
    assert lib.hommx_plan_load_kernel_name(None) == b""
    assert lib.hommx_plan_corrector_kernel_name(None) == b""
