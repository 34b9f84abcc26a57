"""``BaseHMM.solve_nonlinear(method="newton")`` on the CPU: a stand-in plan whose ``secant_tangent`` is
tests/secant_tangent_ref.py (the reference's iteration, the analytic element tangent, the reference's solver of the tangent kind).
Newton against the secant loop, the super-linear drop of the history, the identity law, the asymmetry WARNING, the new RuntimeError
and a two-rank gloo run (no GPU needed)."""

import logging
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import secant_tangent_ref as TR
from hommx_amd import hmm, mesh
from hommx_amd.batch import SecantResult
from test_reconstruct_host import ReconOraclePlan
from test_secant_hmm_host import SecantOraclePlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TangentOraclePlan(SecantOraclePlan):
    """``secant`` of the parent; ``secant_tangent`` adds D of secant_tangent_ref.tangent with the analytic derivative ``dlaw``."""

    def __init__(self, dim, n, kind, dlaw):
        super().__init__(dim, n, kind)
        self.dlaw, self.tangent_calls = dlaw, []
        self.tangent_kind = TR.TANGENT_KIND[kind]
        self.sibling = ReconOraclePlan(dim, n, self.tangent_kind)  # what the solver keeps as its sibling plan: matched by its kind

    def secant_tangent(self, coef, xi, law, tangent_plan, M=None, rows=None, points=None, max_iter=50, tol=1e-10, relax=1.0, **kw):
        self.tangent_calls.append(len(coef))
        assert tangent_plan is self.sibling
        rs = [TR.tangent(self.kind, self.dim, law, self.dlaw, coef[k], xi[k], None if M is None else M[k], n=self.n, x=rows[k, :3], y=points,
                         max_iter=max_iter, tol=tol, relax=relax) for k in range(len(coef))]
        col = lambda name, dtype=float: np.array([r[name] for r in rs], dtype=dtype)
        return SecantResult(np.stack([r["A"] for r in rs]), np.stack([r["mean_flux"] for r in rs]), col("rounds", np.int64), col("change"),
                            col("status", np.int64), np.zeros(len(coef), np.int32), tangent=np.stack([r["D"] for r in rs]),
                            asymmetry=col("asymmetry"), tangent_info=np.zeros(len(coef), np.int32))


IDENTITY = (hmm.SecantLaw("c[0]"), lambda e, b: np.zeros((len(e), 1, e.shape[1])))


def _solver(law_pair=None, A=None, f=40.0, nx=3, n=4):
    law, dlaw = law_pair or TR.potential_law("poisson", 2)
    A = A or (lambda x, y: 1.0 + 0.3 * np.sin(2 * np.pi * y[0]) + 0.1 * x[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: f + x[0], mesh.create_unit_square(n, n), 0.01, quadrature_degree=3)
    h._plan = TangentOraclePlan(2, n, "poisson", dlaw)
    h._tangent_plan = h._plan.sibling
    return h, law


@pytest.fixture(scope="module")
def runs():
    """One secant and one Newton run to tol = 1e-12, shared."""
    h, law = _solver()
    us = h.solve_nonlinear(law, max_iter=60, tol=1e-12, micro_tol=1e-13, micro_iter=200).x.array.copy()
    secant_history = list(h.nonlinear_history)
    un = h.solve_nonlinear(law, max_iter=60, tol=1e-12, micro_tol=1e-13, micro_iter=200, method="newton").x.array.copy()
    return h, us, secant_history, un, list(h.nonlinear_history)


def test_newton_reaches_the_secant_solution_in_fewer_steps(runs):
    h, us, hs, un, hn = runs
    dev = np.abs(un - us).max() / np.abs(us).max()
    print(f"secant {len(hs)} steps, newton {len(hn)} steps, |u_newton - u_secant| = {dev:.2e} of max |u|")
    print("secant history", ["%.2e" % v for v in hs])
    print("newton history", ["%.2e" % v for v in hn])
    assert dev <= 1e-9
    assert len(hn) < len(hs)
    assert h.tangent_tensors.shape == h.effective_tensors.shape and not np.allclose(h.tangent_tensors, h.effective_tensors, rtol=1e-3)
    assert h._linearisation_load is None and h._needs_reassembly


QUADRATIC_C = 3.0  # the CPU run of this problem: change_{k+1} / change_k^2 = 0.02, 0.01, 1.56 over its four steps; about twice the largest


def test_the_history_drops_super_linearly(runs):
    """Newton: every one of the last three changes is at most C times the square of the one before, C = 3 from the CPU run (history
    5.0e-1, 4.9e-3, 2.5e-7, 1.0e-13; the last entry is still two hundred times the rounding floor of this problem, 5e-16, so it is
    a step of the method and not noise).  The secant loop's history, which drops by a constant factor, does not meet the bound."""
    _, _, hs, _, hn = runs
    assert len(hn) >= 4
    pairs = lambda h: list(zip(h[-4:-1], h[-3:]))
    print("newton history", ["%.3e" % v for v in hn], "ratios", ["%.2f" % (b / a ** 2) for a, b in pairs(hn)])
    for a, b in pairs(hn):
        assert b <= QUADRATIC_C * a ** 2
    assert hn[-1] > 1e-14  # not at the floor: the last comparison says something
    assert all(b > QUADRATIC_C * a ** 2 for a, b in pairs(hs))


def test_a_cell_without_a_tangent_takes_the_secant_step():
    """Status 2 or 3: the tangent is NaN.  Such a cell enters the macro matrix with its secant tensor and no load, so the step stays
    finite; with every cell in that state the Newton step IS the secant step."""
    h, law = _solver()
    real = h._plan.secant_tangent

    def lost(*a, **kw):
        r = real(*a, **kw)
        r.status[:], r.tangent[:], r.asymmetry[:] = 2, np.nan, np.nan
        return r

    h._plan.secant_tangent = lost
    un = h.solve_nonlinear(law, max_iter=2, tol=0.0, method="newton").x.array.copy()
    us = h.solve_nonlinear(law, max_iter=2, tol=0.0).x.array
    assert np.isfinite(un).all() and np.isnan(h.tangent_tensors).all()
    assert np.abs(un - us).max() <= 1e-12 * np.abs(us).max()


def test_the_identity_law_gives_solve_in_one_step_with_the_tangent_equal_to_a_eff():
    h, law = _solver(IDENTITY, f=1.0)
    u = h.solve().x.array.copy()
    linear = h.effective_tensors.copy()
    v = h.solve_nonlinear(law, method="newton", chunk_cells=7)
    assert h._plan.tangent_calls == [7, 7, 4] and not h._plan.secant_calls
    assert len(h.nonlinear_history) == 1 and h.nonlinear_history[0] <= 1e-12
    assert np.abs(v.x.array - u).max() <= 1e-12 * np.abs(u).max()
    assert np.abs(h.tangent_tensors - linear).max() <= 1e-12 * np.abs(linear).max()
    assert np.abs(h.effective_tensors - linear).max() <= 1e-12 * np.abs(linear).max()
    assert np.all(h.secant.asymmetry == 0.0)
    assert np.abs(h.solve().x.array - u).max() <= 1e-12 * np.abs(u).max()  # the linearisation load is gone


def test_the_asymmetry_warning_and_the_new_runtime_error(caplog):
    """A stand-in that reports an asymmetric tangent: one WARNING names the largest value.  An implicit law: RuntimeError."""
    h, law = _solver()
    real = h._plan.secant_tangent

    def skewed(*a, **kw):
        r = real(*a, **kw)
        r.asymmetry = np.linspace(0.0, 0.03125, len(r.asymmetry))
        return r

    h._plan.secant_tangent = skewed
    with caplog.at_level(logging.WARNING):
        h.solve_nonlinear(law, max_iter=30, tol=1e-9, method="newton")
    warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "not symmetric" in warnings[0] and "3.125e-02" in warnings[0] and "quasi-Newton" in warnings[0]
    with pytest.raises(RuntimeError, match=r"explicit law; this one reads s\[0\]"):
        h.solve_nonlinear(hmm.SecantLaw("c[0]/(1 + s[0]**2)"), method="newton")
    with pytest.raises(ValueError, match="method must be"):
        h.solve_nonlinear(law, method="bfgs")
    caplog.clear()
    h._plan.secant_tangent = real
    with caplog.at_level(logging.WARNING):
        h.solve_nonlinear(law, max_iter=30, tol=1e-9, method="newton")
    assert not [r for r in caplog.records if r.levelno == logging.WARNING]


# -- two ranks over gloo -----------------------------------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    h, law = _solver()
    u = h.solve_nonlinear(law, max_iter=3, tol=0.0, method="newton").x.array.copy()
    r = h.secant
    q.put((rank, {"u": u, "A": r.A_eff, "D": r.tangent, "asym": r.asymmetry, "flux": r.mean_flux, "rounds": r.rounds, "status": r.status,
                  "cells": h._plan.tangent_calls, "history": h.nonlinear_history}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_newton():
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
    h, law = _solver()
    u = h.solve_nonlinear(law, max_iter=3, tol=0.0, method="newton").x.array
    for r in (0, 1):
        assert got[r]["cells"] == [9, 9, 9]  # every rank linearised only its 9 of the 18 cells, in each of the three macro steps
        assert np.array_equal(got[r]["u"], u) and got[r]["history"] == h.nonlinear_history
        for name, want in (("A", h.secant.A_eff), ("D", h.secant.tangent), ("asym", h.secant.asymmetry), ("flux", h.secant.mean_flux),
                           ("rounds", h.secant.rounds), ("status", h.secant.status)):
            assert np.array_equal(got[r][name], want), name
