"""``BaseHMM.solve_nonlinear`` on the CPU: a stand-in plan whose ``secant`` is tests/secant_ref.py (the same rounds on the oracle's
correctors), the identity law against ``solve()``, the macro Kacanov loop against one assembled here from per-cell scalars, the three
``RuntimeError``s, the WARNING, and a two-rank gloo run through ``run_sharded`` (no GPU needed)."""

import logging
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import secant_ref as S
from hommx_amd import hmm, mesh
from hommx_amd.batch import SecantResult
from test_reconstruct_host import ReconOraclePlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOFT = "c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"


class SecantOraclePlan(ReconOraclePlan):
    """Answers secant() with secant_ref.iterate on the oracle's correctors; records the batch sizes and limits it was given."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.secant_calls = []

    def secant(self, coef, xi, law, M=None, rows=None, points=None, max_iter=50, tol=1e-10, relax=1.0, coef_start=None, fields=False,
               values=False, return_coef=False):
        self.secant_calls.append((len(coef), np.shape(rows), np.shape(points), max_iter, tol, relax))
        solve = S.solver(self.kind, self.dim, self.n)
        rs = [S.iterate(solve, law, coef[k], xi[k], None if M is None else M[k], rows[k, :3], points, rows[k, 3:] if law.n_fields else None,
                        max_iter, tol, relax) for k in range(len(coef))]
        return SecantResult(np.stack([r["A"] for r in rs]), np.stack([r["mean_flux"] for r in rs]), np.array([r["rounds"] for r in rs]),
                            np.array([r["change"] for r in rs]), np.array([r["status"] for r in rs]), np.zeros(len(coef), np.int32))


def _solver(A=None, f=40.0, nx=4, n=4):
    A = A or (lambda x, y: 1.0 + 0.0 * x[0] * y[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: f + 0.0 * x[0], mesh.create_unit_square(n, n), 0.01, quadrature_degree=3)
    h._plan = SecantOraclePlan(2, n, "poisson")
    return h


def test_the_identity_law_stops_after_one_macro_step_and_equals_solve():
    A = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * x[0]) + 0.9 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1])
    h = _solver(A, f=1.0)
    u = h.solve().x.array.copy()
    linear = h.effective_tensors.copy()
    v = h.solve_nonlinear(hmm.SecantLaw("c[0]"), chunk_cells=13)
    n = h._msh.num_cells
    assert [c[0] for c in h._plan.secant_calls] == [13, 13, n - 26]
    assert all(c[1:] == ((c[0], 3), (32, 2), 50, 1e-10, 1.0) for c in h._plan.secant_calls)  # the midpoints, the centroids, the defaults
    assert len(h.nonlinear_history) == 1 and h.nonlinear_history[0] <= 1e-12
    assert np.abs(v.x.array - u).max() <= 1e-12 * np.abs(u).max()
    assert np.abs(h.effective_tensors - linear).max() <= 1e-12 * np.abs(linear).max()
    assert np.array_equal(h.secant.rounds, np.ones(n, dtype=np.int64)) and not h.secant.status.any() and np.array_equal(h.secant.cells, np.arange(n))
    # marked for reassembly: the next solve() is the linear one again
    assert h._needs_reassembly and np.abs(h.solve().x.array - u).max() <= 1e-12 * np.abs(u).max()


def test_every_macro_iterate_is_that_of_the_kacanov_loop_of_the_macro_problem():
    """A homogeneous micro coefficient: the secant tensor of a cell is a(|grad u|) I, so the macro iterates are those of the Kacanov
    loop of -div(a(|grad u|) grad u) = f on P1 elements, assembled here from per-cell scalars through the solver's own helpers."""
    h = _solver()
    law = hmm.SecantLaw(SOFT)
    cells = np.arange(h._msh.num_cells)
    u = h.solve().x.array.copy()
    for k in range(1, 6):
        xi = h._macro_strains(cells, u)
        a = 0.5 + 0.5 / (1 + (xi**2).sum(axis=1))
        h._set_macro_matrix(h._local_stiffness_from_tensors(cells, a[:, None, None] * np.eye(2)))
        u = h.solve().x.array.copy()
        h._needs_reassembly = True
        got = h.solve_nonlinear(law, max_iter=k, tol=0.0).x.array
        dev = np.abs(got - u).max() / np.abs(u).max()
        assert dev <= 1e-10, (k, dev)
        assert len(h.nonlinear_history) == k
    assert h.nonlinear_history[0] > 1e-3 and h.nonlinear_history[-1] < h.nonlinear_history[0]  # the load is large enough for the law to matter
    assert np.abs(h.effective_tensors - (a[:, None, None] * np.eye(2))).max() <= 1e-10
    assert np.all(h.secant.rounds <= 2) and (h.secant.rounds == 2).any()  # a cell without a gradient stops at once
    assert np.abs(h.secant.mean_flux - a[:, None] * xi).max() <= 1e-10
    start = h.solve_nonlinear(law, max_iter=1, tol=0.0, u0=u).x.array  # u0: one more step from the fifth iterate
    assert np.abs(start - u).max() <= 10 * h.nonlinear_history[0] * np.abs(u).max() and not np.array_equal(start, u)


def test_the_three_runtime_errors():
    h = _solver()
    with pytest.raises(RuntimeError, match="field_values"):
        h.solve_nonlinear(hmm.SecantLaw("c[0]*f[0]", fields=1))
    h.set_polarisation(np.zeros((32, 2)))
    with pytest.raises(RuntimeError, match="polarisation"):
        h.solve_nonlinear(hmm.SecantLaw(SOFT))
    per = hmm.PoissonPeriodicHMM(mesh.create_unit_square(3, 3), lambda y: 1.0 + 0.0 * y[0], lambda x: 1.0 + 0.0 * x[0],
                                 mesh.create_unit_square(4, 4), 0.01)
    with pytest.raises(RuntimeError, match="PoissonPeriodicHMM has no solve_nonlinear"):
        per.solve_nonlinear(hmm.SecantLaw(SOFT))


def test_fields_of_the_law_reach_the_plan_and_one_warning_counts_the_statuses(caplog):
    h = _solver(nx=3)
    n = h._msh.num_cells
    law = hmm.SecantLaw("c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))*f[0]", fields=("damage",))
    with caplog.at_level(logging.WARNING):
        h.solve_nonlinear(law, max_iter=30, tol=1e-9, field_values=np.linspace(0.5, 1.0, n))
    assert not caplog.records and h.nonlinear_history[-1] <= 1e-9 and not h.secant.status.any()
    assert all(c[1] == (c[0], 4) for c in h._plan.secant_calls)
    plain = h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=30, tol=1e-9).x.array.copy()
    assert not np.array_equal(plain, h.solve_nonlinear(law, max_iter=30, tol=1e-9, field_values=np.linspace(0.5, 1.0, n)).x.array)
    caplog.clear()
    h = _solver(lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]) + 0.0 * x[0], nx=3)  # heterogeneous: two rounds at tol 0 do not settle a cell
    with caplog.at_level(logging.WARNING):
        h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=2, tol=1e-14, micro_iter=2, micro_tol=0.0)
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1
    text = warnings[0].getMessage()
    assert "did not converge" in text and "after 2 macro steps" in text and "micro cells by status" in text
    stopped = int((h.secant.status == 1).sum())  # the cells whose two rounds did not settle (a gradient along the layers settles at once)
    assert stopped > 0 and f"1: {stopped}" in text and f"0: {n - stopped}" in text


# -- two ranks over gloo -----------------------------------------------------------------------------------------------------------------
def _gloo_problem():
    A = lambda x, y: 1.0 + 0.3 * np.sin(2 * np.pi * y[0]) + 0.1 * x[0]
    h = hmm.PoissonHMM(mesh.create_unit_square(3, 3), A, lambda x: 30.0 + x[0], mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
    h._plan = SecantOraclePlan(2, 4, "poisson")
    return h


def _gloo_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    h = _gloo_problem()
    u = h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=3, tol=0.0).x.array.copy()
    r = h.secant
    q.put((rank, {"u": u, "A": r.A_eff, "flux": r.mean_flux, "rounds": r.rounds, "change": r.change, "status": r.status, "info": r.info,
                  "cells": [c[0] for c in h._plan.secant_calls], "history": h.nonlinear_history}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_solve_nonlinear():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    h = _gloo_problem()
    u = h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=3, tol=0.0).x.array
    for r in (0, 1):
        assert got[r]["cells"] == [9, 9, 9]  # every rank iterated only its 9 of the 18 cells, in each of the three macro steps
        assert np.array_equal(got[r]["u"], u) and got[r]["history"] == h.nonlinear_history
        for name, want in (("A", h.secant.A_eff), ("flux", h.secant.mean_flux), ("rounds", h.secant.rounds), ("change", h.secant.change),
                           ("status", h.secant.status), ("info", h.secant.info)):
            assert np.array_equal(got[r][name], want), name
