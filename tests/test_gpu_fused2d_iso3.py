"""The unstratified 32-wide fused kernel at three waves per SIMD: band matrices built in the registers, S_last parked in LDS (-m gpu).

The kernel k_poisson2d_fused<32, false, true> has no staging matrix: its prologue writes S_last, T_0 and W_0 into the registers under lane
masks, and its twelve S_last accumulator registers live in LDS between two steps, so that twelve workgroups share a CU.  Checked here:
  - the specialised path (M = None) against the general one (M = the identity as an array) bit for bit at n = 18, 19, 20, 29, 30 -- with 17, 31, 32
    of test_gpu_fused2d_iso.py every residue of the first real index p0 = 32 - n modulo 4 at both ends of tile 0, i.e. every lane position of
    the wrap-around entries;
  - a negative and a NaN coefficient at n = 20: the same flags as the general path, the good cells bit-equal;
  - 3,200 cells at n = 32 (more than 256 CUs x 12 resident workgroups) of 16 distinct coefficient sets: a cell's bits do not depend on where it
    sits in the batch nor on what shares its CU.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [18, 19, 20, 29, 30]


def plan(n):
    from hommx_amd import MicroCellPlan

    p = MicroCellPlan(2, n, "poisson")
    assert p.kernel == "fused2d"
    return p


def eye(nc):
    return np.broadcast_to(np.eye(2), (nc, 2, 2)).copy()


def cells(n, rng):
    coef = np.exp(rng.uniform(np.log(0.05), np.log(5.0), size=(7, 2 * n * n)))
    coef[6] = np.where(rng.uniform(size=2 * n * n) < 0.5, 1e-4, 1e3)
    return coef


@pytest.mark.parametrize("n", SIZES)
def test_specialised_equals_general_bitwise(n, rng):
    p = plan(n)
    coef = cells(n, rng)
    A, info = p.solve(coef, return_info=True)
    Ag, infog = p.solve(coef, eye(len(coef)), return_info=True)
    assert np.isfinite(A).all()
    assert np.array_equal(A, Ag)
    assert np.array_equal(info, infog)


def test_bad_cells_flagged_as_general():
    n = 20
    p = plan(n)
    coef = np.ones((5, 2 * n * n))
    coef[0] = 0.7
    coef[1] = -1.0
    coef[3, 5] = np.nan
    coef[4, ::3] = 2.5
    bad = np.array([False, True, False, True, False])
    A, info = p.solve(coef, return_info=True)
    Ag, infog = p.solve(coef, eye(5), return_info=True)
    assert np.array_equal(info, infog)
    assert np.all(info[bad] > 0) and np.all(info[~bad] == 0)
    assert np.isfinite(A[~bad]).all()
    assert np.array_equal(A[~bad], Ag[~bad])


def test_position_independent_with_every_slot_resident(rng):
    n, nsets, ncells = 32, 16, 3200
    p = plan(n)
    base = np.exp(rng.uniform(np.log(0.05), np.log(5.0), size=(nsets, 2 * n * n)))
    base[nsets - 1] = np.where(rng.uniform(size=2 * n * n) < 0.5, 1e-4, 1e3)
    coef = np.ascontiguousarray(np.tile(base, (ncells // nsets, 1)))
    A, info = p.solve(coef, return_info=True)
    assert not info.any() and np.isfinite(A).all()
    A = A.reshape(ncells // nsets, nsets, 2, 2)
    assert np.array_equal(A, np.broadcast_to(A[0], A.shape))  # the same coefficients give the same bits wherever the cell sits
    A16, info16 = p.solve(base, return_info=True)
    assert not info16.any()
    assert np.array_equal(A[0], A16)                          # and the first 16 equal the same 16 as a batch of their own
