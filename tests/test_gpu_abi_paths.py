"""The pipelined path of hommx_solve_batch (batches from two copy chunks up: coefficient chunks stream in on one stream while the other
solves the previous one) == hommx_solve_batch_device on the same data uploaded by the test, bit for bit (-m gpu)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORCE_BLOCKED = 1  # HOMMX_FLAG_FORCE_BLOCKED


# cells per copy chunk of hommx_solve_batch at n_micro = 4: 2048 on the fused family; the blocked family's 256 MB / (32 doubles) clamps to 4096
@pytest.mark.parametrize("flags,kernel_is_fused,chunk", [(0, True, 2048), (FORCE_BLOCKED, False, 4096)])
def test_pipelined_host_entry_equals_device_entry(flags, kernel_is_fused, chunk):
    import torch

    from hommx_amd import MicroCellPlan

    p = MicroCellPlan(2, 4, "poisson", flags=flags)
    assert (p.kernel == "fused2d") == kernel_is_fused
    nc = 2 * chunk + 1  # two full chunks and a tail of one cell
    rng = np.random.default_rng(20261018)
    coef = rng.uniform(0.5, 2.0, (nc, p.n_el))
    M = np.eye(2)[None] + 0.2 * rng.standard_normal((nc, 2, 2))
    A, info = p.solve(coef, M, return_info=True)
    assert np.all(info == 0)

    dev = torch.device("cuda", p.device)
    d_coef, d_M = torch.from_numpy(coef).to(dev), torch.from_numpy(M).to(dev)
    d_A = torch.zeros((nc, 2, 2), dtype=torch.float64, device=dev)
    d_info = torch.full((nc,), -7, dtype=torch.int32, device=dev)
    p.solve_device(nc, d_coef.data_ptr(), d_M.data_ptr(), d_A.data_ptr(), d_info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_info.cpu().numpy(), info)
    assert np.array_equal(d_A.cpu().numpy(), A)
