"""The argument checks of the solve entry points of the C ABI on the CPU: every check runs before the plan's device is made current and
reads nothing of the plan but its descriptor, so plan-shaped memory that holds only a hommx_plan_desc is enough to reach each of them.
Every call here is a faulty one (or an empty batch): none may get past the checks (no GPU needed)."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib
from test_reconstruct_source_host import _fake_plan

KINDS = [_lib.KIND_POISSON_SCALAR, _lib.KIND_POISSON_MATRIX, _lib.KIND_ELASTICITY_ISO]
AFFINE, RECIPROCAL = _lib.SAMPLER_AFFINE, _lib.SAMPLER_RECIPROCAL


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@pytest.fixture(scope="module")
def ptr():
    buf = np.zeros(64)
    yield buf.ctypes.data
    del buf


# entry -> (the arguments after n_cells, every pointer set (P stands for one); the positions of the required pointers; the entry's own text)
P = "P"
ENTRIES = {
    "hommx_solve_batch": ((P, None, P, None), (0, 2), "null coef / A_eff"),
    "hommx_solve_batch_device": ((P, None, P, None, None), (0, 2), "null coef / A_eff"),
    "hommx_solve_batch_two_phase": ((P, P, None, P, None), (0, 1, 3), "null mask / values / A_eff"),
    "hommx_solve_batch_two_phase_device": ((P, P, None, P, None, None), (0, 1, 3), "null mask / values / A_eff"),
    "hommx_solve_batch_separable": ((AFFINE, 1, P, None, P, None, P, None), (2, 4, 6), "null table / params / A_eff"),
    "hommx_solve_batch_separable_device": ((AFFINE, 1, P, None, P, None, P, None, None), (2, 4, 6), "null table / params / A_eff"),
    "hommx_solve_batch_correctors": ((P, None, P, P, None), (0, 2, 3), "null coef / A_eff / correctors"),
    "hommx_plan_reserve": ((), (), None),
}
DEVICE_ENTRIES = [e for e in ENTRIES if e.endswith("_device")]
SEPARABLE = ["hommx_solve_batch_separable", "hommx_solve_batch_separable_device"]


def _call(lib, entry, plan, n_cells, args, ptr):
    rc = getattr(lib, entry)(plan, n_cells, *[ptr if a is P else a for a in args])
    return rc, lib.hommx_last_error().decode()


def _kinds_of(entry):
    # a separable sampler is defined for two of the kinds: on the third every call fails on the kind (test_separable_restrictions)
    return [k for k in KINDS if entry not in SEPARABLE or k != _lib.KIND_POISSON_MATRIX]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_plan_and_batch_size(lib, ptr, entry):
    args = ENTRIES[entry][0]
    for n_cells in (1, 0, -1):  # a null plan is an error even for an empty batch
        rc, msg = _call(lib, entry, None, n_cells, args, ptr)
        assert rc == -1 and "null plan" in msg, (n_cells, rc, msg)
    for kind in KINDS:
        fake = _fake_plan(kind)
        plan = ctypes.addressof(fake)
        assert lib.hommx_plan_kind(plan) == kind
        rc, msg = _call(lib, entry, plan, -1, args, ptr)
        assert rc == -1 and "negative n_cells" in msg, (kind, rc, msg)
        assert _call(lib, entry, plan, 0, args, ptr)[0] == 0, kind
        assert _call(lib, entry, plan, 0, [None if a is P else a for a in args], ptr)[0] == 0, kind  # an empty batch reads no pointer


@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e][1]])
def test_each_required_pointer(lib, ptr, entry):
    args, required, text = ENTRIES[entry]
    for kind in _kinds_of(entry):
        fake = _fake_plan(kind)
        for k in required:
            bad = list(args)
            bad[k] = None
            rc, msg = _call(lib, entry, ctypes.addressof(fake), 1, bad, ptr)
            assert rc == -1 and msg == text, (kind, k, rc, msg)


@pytest.mark.parametrize("entry", DEVICE_ENTRIES)
def test_batch_too_large_for_one_launch(lib, ptr, entry):
    for kind in _kinds_of(entry):
        fake = _fake_plan(kind)
        rc, msg = _call(lib, entry, ctypes.addressof(fake), 2**31, ENTRIES[entry][0], ptr)
        assert rc == -1 and "too large for one launch" in msg, (kind, rc, msg)


@pytest.mark.parametrize("entry", SEPARABLE)
def test_separable_restrictions(lib, ptr, entry):
    tail = (None,) if entry.endswith("_device") else ()

    def call(kind, family, n_q, weights):
        fake = _fake_plan(kind)
        return _call(lib, entry, ctypes.addressof(fake), 1, (family, n_q, P, weights, P, None, P, None) + tail, ptr)

    rc, msg = call(_lib.KIND_POISSON_MATRIX, AFFINE, 1, None)
    assert rc == -1 and "separable samplers are defined for the scalar Poisson and the isotropic elasticity kinds" in msg, (rc, msg)
    rc, msg = call(_lib.KIND_ELASTICITY_ISO, RECIPROCAL, 3, P)
    assert rc == -1 and "isotropic elasticity kind takes the affine sampler only" in msg, (rc, msg)
    rc, msg = call(_lib.KIND_POISSON_SCALAR, 5, 1, None)
    assert rc == -1 and "unknown sampler family 5" in msg, (rc, msg)
    for n_q, weights in ((0, P), (-2, P), (3, None)):
        rc, msg = call(_lib.KIND_POISSON_SCALAR, RECIPROCAL, n_q, weights)
        assert rc == -1 and "reciprocal sampler needs n_q >= 1 and weights" in msg, (n_q, weights, rc, msg)
