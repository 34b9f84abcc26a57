"""Multi-GPU sharding of the macro-cell loop (one process per GPU, torch.distributed over RCCL).

The reference shards the same way across MPI ranks: every rank solves the cell problems of the
macro cells it owns (/root/reference/src/hommx/hmm.py:307-310, docs/usage/usage.md:64-71) and the
results meet in PETSc's MatAssembly stash (hmm.py:325-330, :442).  Here the micro problems never
communicate; the only exchange is ONE all-gather of the effective-tensor field together with the
per-cell info flags (N_c x (t*t + 1) doubles, <= a few MB: latency-bound), so that every rank can
assemble the macro matrix and log failed cells exactly as a single rank would (hmm.py:320-323).

Every rank samples, uploads and solves ONLY its own block of cells; on the RCCL backend the shard
stays in device memory from the solve to the collective (one D2H copy of the gathered field).
"""

from __future__ import annotations

import numpy as np

from .batch import CoefStream, MicroCellPlan


def shard_range(n_cells: int, rank: int, world: int) -> tuple[int, int, int]:
    """Contiguous block partition padded to equal counts: returns (begin, end, per_rank).

    cells_r = [r * ceil(N_c / P), min(N_c, (r+1) * ceil(N_c / P)))  (SURVEY 8(e))."""
    per = -(-n_cells // world)
    b = min(n_cells, rank * per)
    e = min(n_cells, (rank + 1) * per)
    return b, e, per


_selected_device: int | None = None  # the caller's explicit choice (select_device); honoured even when it is ordinal 0


def select_device(device: int | None) -> None:
    """Record the device this rank's plans shall use (and make it torch's current device when torch is loaded and sees a GPU).
    ``torch.cuda.set_device(0)`` alone cannot be told from the untouched default, so a caller that MEANS ordinal 0 under a launcher
    whose LOCAL_RANK says otherwise calls this (or passes ``device=0`` to the solver class).  ``None`` forgets the choice."""
    import sys

    global _selected_device
    _selected_device = None if device is None else int(device)
    torch = sys.modules.get("torch")
    if device is not None and torch is not None and torch.cuda.is_available():
        torch.cuda.set_device(int(device))


def _group_bound_device():
    """Device a process group was bound to with ``init_process_group(..., device_id=...)``: an explicit choice as well."""
    import sys

    dist = sys.modules.get("torch.distributed")
    try:
        if dist is None or not (dist.is_available() and dist.is_initialized()):
            return None
        pg = dist.distributed_c10d._get_default_group()
        dev = getattr(pg, "bound_device_id", None)
        if dev is not None and dev.type == "cuda" and dev.index is not None:
            return int(dev.index)
    except Exception:
        pass
    return None


def default_device(device_count=None) -> int:
    """Device ordinal a rank should use when no ``device=`` was passed.  Resolved LAZILY, at the first solve (a solver may be built
    before ``init_process_group`` / ``torch.cuda.set_device``).  In this order: the ordinal recorded by ``select_device`` (0
    included); the device the default process group is bound to (``device_id=``); the torch device the caller has already selected
    when it is not the untouched default 0; ``LOCAL_RANK % visible devices`` (a launcher that exposes one device per rank through
    HIP_VISIBLE_DEVICES leaves exactly one visible ordinal, 0); else 0."""
    import os
    import sys

    if _selected_device is not None:
        return _selected_device
    bound = _group_bound_device()
    if bound is not None:
        return bound
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        cur = int(torch.cuda.current_device())
        if cur != 0:
            return cur
    lr = os.environ.get("LOCAL_RANK")
    if lr is not None:
        if device_count is None:
            from . import _lib

            device_count = _lib.load().hommx_device_count()
        return int(lr) % max(1, int(device_count))
    return 0


def all_gather_field(local, n_cells: int, group=None):
    """All-gather the per-rank shard of a field.

    ``local`` is a torch tensor [per_rank, ...] (padded shard) on this rank's device (RCCL) or on the
    CPU (gloo); returns the full field [n_cells, ...] on the same device on every rank.
    """
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    per = local.shape[0]
    full = torch.empty((world * per,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(full, local.contiguous(), group=group)
    return full[:n_cells]


FAILED = -777.0  # failure flag of a rank in the packed buffer (its own row: never confused with a cell's info)


class ShardFailure(RuntimeError):
    """Raised on the ranks whose own block was fine when another rank's ``local_solve`` raised."""


def _unpad_index(n_cells: int, per: int, world: int) -> np.ndarray:
    """Positions of the real cells in the concatenation of the padded shards."""
    return np.concatenate([np.arange(r * per, r * per + max(0, min(n_cells, (r + 1) * per) - min(n_cells, r * per)))
                           for r in range(world)])


def run_sharded(t: int, n_cells: int, local_solve, group=None, device=None, shape: tuple | None = None):
    """Solve this rank's block with ``local_solve(b, e) -> (A[e-b, t, t], info[e-b])`` and all-gather both.  ``shape``: the shape of
    one cell's row of the field when it is not (t, t) (the effective polarisation: (t,)).

    ``local_solve`` may return NumPy arrays or torch tensors (on the rank's GPU: the shard then never leaves the device before
    the collective).  The tensors and the info flags travel in ONE packed buffer [per_rank, t*t + 1] (info as a double: small
    integers are exact).  Returns NumPy ``(A_eff[n_cells, t, t], info[n_cells] int32)`` on every rank.
    """
    import torch
    import torch.distributed as dist

    rank, world = dist.get_rank(group), dist.get_world_size(group)
    b, e, per = shard_range(n_cells, rank, world)
    nloc = e - b
    shape = (t, t) if shape is None else tuple(shape)
    tt = int(np.prod(shape))
    A = info = None
    failure = None
    if nloc > 0:
        try:
            A, info = local_solve(b, e)
        except Exception as exc:  # this rank still takes part in the collective; every rank raises after it (below)
            failure = exc
            A = info = None
    on_gpu = torch.is_tensor(A) and A.is_cuda
    if device is None:
        if on_gpu:
            device = A.device
        elif dist.get_backend(group) == "nccl":  # RCCL moves device memory only
            device = torch.device("cuda", default_device())
    elif not isinstance(device, torch.device):
        device = torch.device("cuda", int(device)) if dist.get_backend(group) == "nccl" else None
    # one extra row per rank carries the failure flag, so that ranks agree on an exception instead of waiting for ever
    buf = torch.zeros((per + 1, tt + 1), dtype=torch.float64, device=device if device is not None else "cpu")
    if failure is not None:
        buf[per, tt] = FAILED
    elif nloc > 0:
        At = A if torch.is_tensor(A) else torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64))
        it = info if torch.is_tensor(info) else torch.from_numpy(np.ascontiguousarray(info))
        buf[:nloc, : tt] = At.reshape(nloc, tt).to(buf.device)
        buf[:nloc, tt] = it.to(buf.device, dtype=torch.float64)
    full = all_gather_field(buf, world * (per + 1), group).cpu().numpy().reshape(world, per + 1, tt + 1)
    failed = [r for r in range(world) if full[r, per, tt] == FAILED]
    if failed:
        if failure is not None:
            raise failure
        raise ShardFailure(f"micro-cell solve failed on rank(s) {failed} (see their exceptions); no field was assembled")
    full = full[:, :per].reshape(world * per, tt + 1)[_unpad_index(n_cells, per, world)]
    return full[:, : tt].reshape((n_cells,) + shape).copy(), np.rint(full[:, tt]).astype(np.int32)


def _on_rccl(group=None) -> bool:
    import torch.distributed as dist

    return dist.is_available() and dist.is_initialized() and dist.get_backend(group) == "nccl"


def solve_block(plan, stream: CoefStream, M: np.ndarray | None, group=None):
    """One rank's block of cells through ``plan`` -> (A_eff, info).  A ``MicroCellPlan`` under the RCCL backend: the arrays of the
    stream and ``M`` are uploaded to the plan's device, ``solve_source_device`` runs on torch's current stream and the result stays
    there (torch tensors) until the collective.  Otherwise the host method of ``plan``, with ``return_info=True``."""
    if not (isinstance(plan, MicroCellPlan) and _on_rccl(group)):
        return stream.solve(plan, M, return_info=True)
    import torch

    dev = torch.device("cuda", plan.device)
    held = []  # the uploads, until the launch below is queued (torch frees in stream order)

    def upload(a):
        held.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return held[-1].data_ptr()

    out = torch.empty((len(stream), plan.t, plan.t), dtype=torch.float64, device=dev)
    info = torch.zeros(len(stream), dtype=torch.int32, device=dev)
    stream.solve_device(plan, upload, None if M is None else upload(np.asarray(M, dtype=np.float64)), out.data_ptr(), info.data_ptr(),
                        torch.cuda.current_stream(dev).cuda_stream)
    return out, info


def _solve_sharded(plan, stream: CoefStream, M, group, device, return_info: bool):
    """Every rank solves its block of ``stream`` / ``M`` and the field (and info) is all-gathered; with no process group, the host method
    of ``plan``.  ``plan``: a MicroCellPlan, or any object with ``t`` and the stream's host method (the gloo tests use the CPU oracle)."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return stream.solve(plan, M, return_info=return_info)
    if device is None and isinstance(plan, MicroCellPlan):
        device = plan.device
    A, info = run_sharded(plan.t, len(stream), lambda b, e: solve_block(plan, stream.block(b, e), None if M is None else M[b:e], group),
                          group, device)
    return (A, info) if return_info else A


def solve_sharded(plan, coef: np.ndarray, M: np.ndarray | None, group=None, device=None, return_info: bool = False):
    """Convenience form for callers that hold the whole batch of sampled element means (``_solve_sharded``)."""
    return _solve_sharded(plan, CoefStream.sampled(coef), M, group, device, return_info)


def solve_sharded_two_phase(plan, mask: np.ndarray, values: np.ndarray, M: np.ndarray | None, group=None, device=None,
                            return_info: bool = False):
    """Same for two-phase media: every rank holds the phase mask, the per-cell phase values shard."""
    return _solve_sharded(plan, CoefStream.two_phase(mask, values), M, group, device, return_info)
