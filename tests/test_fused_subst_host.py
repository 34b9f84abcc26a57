"""Correctors of the fused 2D family by substitution on stored block inverses, host side: the recurrence the two kernels
implement, stated in NumPy, against the oracle; the accessor that names a plan's corrector route (CPU only)."""

import ctypes
import os

import numpy as np
import pytest

from fused_subst_ref import correctors


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from hommx_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("n", [3, 4, 5, 16, 17])
def test_recurrence_reproduces_oracle_correctors(n, with_M):
    """Forward pass, u / w sweep without any stored W_j, backward sweep: every sign and the j = n-2 special case."""
    from oracle import hommx_oracle as O

    rng = np.random.default_rng(1000 * n + with_M)
    coef = np.exp(rng.uniform(np.log(0.1), np.log(5.0), size=2 * n * n))
    M = np.eye(2) + 0.3 * rng.standard_normal((2, 2)) if with_M else None
    cp = O.build_cell_problem("poisson", 2, n, coef, M)
    chi = O.solve_correctors(cp)
    chi = chi - chi.mean(axis=0, keepdims=True)
    got = correctors(cp.K, cp.B, n)
    assert np.abs(got - chi).max() <= 1e-10 * np.abs(chi).max()


def test_library_exports_corrector_kernel_name(lib):
    from hommx_amd import _lib

    assert "hommx_plan_corrector_kernel_name" in _lib.EXPORTED_SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "hommx_plan_corrector_kernel_name")


def test_corrector_kernel_name_of_a_null_plan(lib):
    """As hommx_plan_kernel_name and hommx_plan_route_detail: the empty string."""
    assert lib.hommx_plan_corrector_kernel_name(None) == b""
    assert lib.hommx_plan_kernel_name(None) == b"" and lib.hommx_plan_route_detail(None) == b""
