"""``BaseHMM.solve_nonlinear`` with a law that has history variables, on the CPU: a stand-in plan whose ``secant`` /
``secant_tangent`` are tests/history_ref.py (the rounds of secant_ref with the frozen history, on the oracle's correctors), in the
manner of test_secant_hmm_host.py.  Three load steps with ``commit_history``, a call without a commit reproducing the one before,
both methods, the ``RuntimeError``s, ``reset_history``, and two gloo ranks each holding the history of its own block.  No GPU."""

import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import history_ref as H
import recon_ref as R
from hommx_amd import fem, hmm, mesh
from hommx_amd.batch import SecantResult
from test_reconstruct_host import ReconOraclePlan
from test_secant_hmm_host import SecantOraclePlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQ = "sqrt(e[0]**2 + e[1]**2)"
N_MICRO = 4


def damage_law(**kw):
    return hmm.SecantLaw(f"c[0]*(1 - 0.5*(1 - exp(-max(h[0], {EQ})/0.7)))", history=[f"max(h[0], {EQ})"], history_names=("kappa",), **kw)


class HistoryOraclePlan(SecantOraclePlan):
    """``secant(history=)`` is history_ref.iterate per cell; ``secant_tangent(history=)`` adds D, the linear cell problem of the
    oracle on ``SecantLaw.host_tangent(history=)``.  Records the history blocks it was given."""

    tangent_kind = "poisson_matrix"

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.history_calls = []
        self.sibling = ReconOraclePlan(dim, n, self.tangent_kind)  # what the solver keeps as its sibling plan: matched by its kind

    def secant(self, coef, xi, law, M=None, rows=None, points=None, max_iter=50, tol=1e-10, relax=1.0, history=None, tangent=False):
        assert history is not None and history.shape == (len(coef), coef.shape[1], law.n_history)
        self.secant_calls.append((len(coef), np.shape(rows), np.shape(points), max_iter, tol, relax))
        self.history_calls.append(history.copy())
        solve = H.solver(self.kind, self.dim, self.n)
        rs = [H.iterate(solve, law, coef[k], xi[k], history[k], None if M is None else M[k], rows[k, :3], points, None, max_iter, tol, relax)
              for k in range(len(coef))]
        out = SecantResult(np.stack([r["A"] for r in rs]), np.stack([r["mean_flux"] for r in rs]), np.array([r["rounds"] for r in rs]),
                           np.array([r["change"] for r in rs]), np.array([r["status"] for r in rs]), np.zeros(len(coef), np.int32),
                           history=np.stack([r["history"] for r in rs]))
        if tangent:
            D = []
            for k, r in enumerate(rs):
                T, _ = law.host_tangent(r["s"][None], r["coef"][None], coef[k][None], rows[k, None, :3], points, history=history[k][None])
                stream = np.stack([T[0, :, 0, 0], T[0, :, 1, 1], T[0, :, 0, 1]], axis=-1)  # the component order of poisson_matrix
                D.append(R.structured("poisson_matrix", self.dim, self.n, stream, None if M is None else M[k], xi[k])["A"])
            out.tangent, out.asymmetry = np.stack(D), np.zeros(len(coef))
        return out

    def secant_tangent(self, coef, xi, law, tangent_plan, M=None, **kw):
        assert tangent_plan is self.sibling
        return self.secant(coef, xi, law, M, tangent=True, **kw)


def _solver(nx=2, n=N_MICRO, f=0.0):
    A = lambda x, y: 1.0 + 0.3 * np.sin(2 * np.pi * y[0]) + 0.1 * x[0]
    # no source: the boundary values alone drive the macro gradient, so scaling them loads and unloads every cell
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: f + 0.0 * x[0], mesh.create_unit_square(n, n), 0.01, quadrature_degree=3)
    h._plan = HistoryOraclePlan(2, n, "poisson")
    h._tangent_plan = h._plan.sibling
    return h


def _bcs(h, scale):
    """u = scale * x0 on the boundary: the load steps scale the macro gradient."""
    V = h.function_space
    nodes = hmm._box_boundary_nodes(V.mesh)
    g = fem.Function(V)
    g.x.array[:] = scale * V.mesh.geometry.x[:, 0]
    return [fem.dirichletbc(g, nodes, V)]


def _steps(h, law, scales, method="secant", commit=True):
    """solve_nonlinear at every scale, each from the solution before; -> the solutions and the histories after each step."""
    us, hs, u = [], [], None
    for scale in scales:
        h.set_boundary_conditions(_bcs(h, scale))
        u = h.solve_nonlinear(law, max_iter=40, tol=1e-10, micro_tol=1e-12, method=method, u0=u).x.array.copy()
        assert not h.secant.status.any() and h.nonlinear_history[-1] <= 1e-10
        if commit:
            h.commit_history()
        us.append(u)
        hs.append((None if h.history is None else h.history.copy(), h.history_trial.copy()))
    return us, hs


@pytest.fixture(scope="module")
def path():
    h, law = _solver(), damage_law()
    us, hs = _steps(h, law, (1.0, 0.5, 1.5))
    return h, law, us, hs


def test_three_load_steps_with_commit_history(path):
    h, law, us, hs = path
    n, n_el = h._msh.num_cells, 2 * N_MICRO**2
    assert h.history.shape == (n, n_el, 1) and np.array_equal(h.history_cells, np.arange(n))
    load, unload, reload_ = (s[0] for s in hs)
    assert (load > 0).all()  # every element has seen a strain
    assert np.array_equal(unload, load)  # unloading: not a bit of the history changes
    assert (reload_ >= load).all() and (reload_ > load).mean() > 0.9  # reloading: it grows
    # every macro step of a load step got the same frozen history: the committed one
    calls = h._plan.history_calls
    first = [i for i, c in enumerate(calls) if not c.any()]  # the steps of the first load step start from history_initial = 0
    assert first == list(range(len(first))) and len(first) >= 2
    assert all(np.array_equal(c, load) for c in calls[len(first):] if np.array_equal(c[0], load[0]))
    # the unloaded response is the linear one on the damaged coefficient: one more macro step does not move it
    assert np.abs(us[1]).max() > 0 and not np.array_equal(us[0], us[1])


def test_without_commit_history_the_second_call_reproduces_the_first():
    h, law = _solver(), damage_law()
    (u1,), ((state, trial1),) = _steps(h, law, (1.0,), commit=False)
    assert not state.any() and trial1.any()  # the state is still history_initial
    h.set_boundary_conditions(_bcs(h, 1.0))
    u2 = h.solve_nonlinear(law, max_iter=40, tol=1e-10, micro_tol=1e-12).x.array
    assert np.array_equal(u1, u2) and np.array_equal(h.history_trial, trial1) and not h.history.any()
    h.commit_history()
    assert np.array_equal(h.history, trial1)


def test_newton_and_secant_agree_along_the_path(path):
    _, law, us, hs = path
    h = _solver()
    un, hn = _steps(h, law, (1.0, 0.5, 1.5), method="newton")
    for k in range(3):
        dev = np.abs(un[k] - us[k]).max() / np.abs(us[k]).max()
        print("step", k, "newton against secant", dev)
        assert dev <= 1e-8
        assert np.abs(hn[k][0] - hs[k][0]).max() <= 1e-8 * np.abs(hs[k][0]).max()
    assert np.array_equal(hn[1][0], hn[0][0])


def test_history_initial_and_reset_history():
    h, law = _solver(), damage_law(history_initial=0.8)
    h.set_boundary_conditions(_bcs(h, 0.2))
    h.solve_nonlinear(law, max_iter=40, tol=1e-10)
    n, n_el = h._msh.num_cells, 2 * N_MICRO**2
    assert np.array_equal(h.history, np.full((n, n_el, 1), 0.8))
    assert np.array_equal(h.history_trial, h.history)  # a small load under a large initial damage driver: unloading everywhere
    h.reset_history()
    assert h.history is None and h.history_trial is None
    with pytest.raises(RuntimeError, match="commit_history"):
        h.commit_history()
    values = np.linspace(0.1, 0.9, n * n_el).reshape(n, n_el)
    h.reset_history(values)
    assert np.array_equal(h.history[:, :, 0], values)
    h.solve_nonlinear(law, max_iter=40, tol=1e-10)
    assert np.array_equal(h._plan.history_calls[-1][:, :, 0], values)  # the law's history_initial is not read once a state exists
    with pytest.raises(ValueError, match="expected"):
        h.reset_history(np.zeros((n, n_el + 1, 1)))


def test_the_runtime_errors():
    h, law = _solver(), damage_law()
    h.set_boundary_conditions(_bcs(h, 1.0))
    h.solve_nonlinear(law, max_iter=2, tol=0.0)
    two = hmm.SecantLaw("c[0]/(1 + h[0] + h[1])", history=[f"max(h[0], {EQ})", "h[1] + 1"])
    with pytest.raises(RuntimeError, match="reset_history"):  # another law's n_history
        h.solve_nonlinear(two, max_iter=2, tol=0.0)
    h._cell_mesh = mesh.create_unit_square(N_MICRO + 1, N_MICRO + 1)  # a changed micro mesh
    with pytest.raises(RuntimeError, match="reset_history"):
        h.solve_nonlinear(law, max_iter=2, tol=0.0)
    fresh = _solver()
    with pytest.raises(RuntimeError, match="commit_history"):
        fresh.commit_history()
    fresh.set_polarisation(np.zeros((2 * N_MICRO**2, 2)))
    with pytest.raises(RuntimeError, match="polarisation"):
        fresh.solve_nonlinear(law)


# -- two ranks over gloo -----------------------------------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    h, law = _solver(), damage_law()
    us, hs = _steps(h, law, (1.0, 0.5))
    q.put((rank, {"u": us, "history": h.history, "trial": h.history_trial, "cells": h.history_cells,
                  "sizes": sorted({len(c) for c in h._plan.history_calls})}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_each_hold_the_history_of_their_own_block(path):
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
    _, _, us, hs = path
    n = 8
    for r in (0, 1):
        block = np.arange(4 * r, 4 * (r + 1))
        assert np.array_equal(got[r]["cells"], block) and got[r]["sizes"] == [4]  # nothing of the history is gathered
        assert got[r]["history"].shape == (4, 2 * N_MICRO**2, 1)
        assert np.array_equal(got[r]["history"], hs[1][0][block]) and np.array_equal(got[r]["trial"], hs[1][1][block])
        for k in range(2):
            assert np.array_equal(got[r]["u"][k], us[k])
    assert n == len(hs[0][0])
