"""The unstratified path of the fused 2D kernel (k_poisson2d_fused<NB, false, true>) == the general path, bit for bit (-m gpu).

M = None takes the specialised kernel (E diagonal, no neighbour exchange); M = the identity, passed as an array, reaches the general kernel
(api.hip hands a non-null d_M through, batch.py drops it only for None) and computes the same cells with every e1 term an exact zero.  The two
must agree under np.array_equal (which lets the sign of an exact zero differ, nothing else).  Sizes: both block sizes (NB = 16 / 32), no padding
(n = NB), the widest padding (n = 17), first real index not a multiple of four (n = 3, 5, 15, 17, 31); cells: six of log-uniform coefficients in
[0.05, 5] and one two-valued cell of contrast 1e7.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 5, 15, 16, 17, 31, 32]


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


def test_specialised_equals_general_bitwise_device_entry(rng):
    import torch

    n = 17
    p = plan(n)
    coef = cells(n, rng)
    nc = len(coef)
    dc = torch.from_numpy(coef).cuda()
    dM = torch.from_numpy(eye(nc)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for mptr in (None, dM.data_ptr()):
        out = torch.empty(nc, 2, 2, dtype=torch.float64, device="cuda")
        info = torch.full((nc,), -1, dtype=torch.int32, device="cuda")
        p.solve_device(nc, dc.data_ptr(), mptr, out.data_ptr(), info.data_ptr(), stream)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), info.cpu().numpy()))
    assert np.isfinite(res[0][0]).all()
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][0], p.solve(coef))  # and the host entry takes the same path


@pytest.mark.parametrize("n", [32, 12])
def test_sampler_modes_equal_general_bitwise(n, rng):
    """Two-phase, affine and reciprocal (three quadrature points) sources: every CoefSource mode dispatches on M alone."""
    p = plan(n)
    nc = 5
    M = eye(nc)
    mask = rng.uniform(size=p.n_el) < 0.4
    values = rng.uniform(0.2, 4.0, size=(nc, 2))
    A, info = p.solve_two_phase(mask, values, return_info=True)
    Ag, infog = p.solve_two_phase(mask, values, M, return_info=True)
    assert np.isfinite(A).all() and not info.any()
    assert np.array_equal(A, Ag) and np.array_equal(info, infog)

    params = np.stack([rng.uniform(2.0, 3.0, size=nc), rng.uniform(0.2, 1.0, size=nc)], axis=1)  # a + b g > 0 for |g| <= 1
    for family, table, w in (("affine", rng.uniform(-1.0, 1.0, size=p.n_el), None),
                             ("reciprocal", rng.uniform(-1.0, 1.0, size=(p.n_el, 3)), np.array([0.25, 0.5, 0.25]))):
        A, info = p.solve_separable(family, table, w, params, return_info=True)
        Ag, infog = p.solve_separable(family, table, w, params, M, return_info=True)
        assert np.isfinite(A).all() and not info.any()
        assert np.array_equal(A, Ag) and np.array_equal(info, infog)


@pytest.mark.parametrize("n", [16, 32])
def test_failure_flags_agree(n):
    """A negative-coefficient cell and a cell holding a NaN (the inputs of test_edge_cases): both paths flag exactly those, the good cells agree."""
    p = plan(n)
    coef = np.ones((5, 2 * n * n))
    coef[0] = 0.7
    coef[1] = -1.0
    coef[3, 5] = np.nan
    coef[4, ::3] = 2.5
    bad = np.array([False, True, False, True, False])
    A, info = p.solve(coef, return_info=True)
    Ag, infog = p.solve(coef, eye(5), return_info=True)
    for i_ in (info, infog):
        assert np.all(i_[bad] > 0) and np.all(i_[~bad] == 0)
    assert np.isfinite(A[~bad]).all()
    assert np.array_equal(A[~bad], Ag[~bad])
