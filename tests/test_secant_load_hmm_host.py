"""``BaseHMM.solve_nonlinear(load=True)`` on the CPU: a stand-in plan whose ``secant`` / ``secant_tangent`` beside a load
are tests/secant_load_ref.py.  The identity law against ``solve()`` with the same eigenstrain, every macro iterate of both methods
against a NumPy loop assembled here from per-cell closed forms, the two ``RuntimeError``s, and a two-rank gloo run (no GPU needed)."""

import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import secant_load_ref as SL
import secant_tangent_ref as TR
from hommx_amd import hmm, mesh
from hommx_amd.batch import SecantResult
from test_loads_host import LoadOraclePlan
from test_reconstruct_host import ReconOraclePlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAW, DLAW = TR.potential_law("poisson", 2)  # c[0] (0.5 + 0.5 / (1 + |e|^2))
IDENTITY = (hmm.SecantLaw("c[0]"), lambda e, b: np.zeros((len(e), 1, e.shape[1])))


class LoadSecantOraclePlan(LoadOraclePlan):
    """``loads`` of the parent (what ``solve()`` asks for); ``secant`` and ``secant_tangent`` with ``P`` answer with secant_load_ref.
    It has no ``load_sources``: the solver hands it sampled arrays, an eigenstrain as it is."""

    def __init__(self, dim, n, kind, dlaw):
        super().__init__(dim, n, kind)
        self.dlaw, self.secant_calls = dlaw, []
        self.tangent_kind = TR.TANGENT_KIND[kind]
        self.sibling = ReconOraclePlan(dim, n, self.tangent_kind)

    def _rounds(self, coef, xi, law, M, rows, points, max_iter, tol, relax, P, per_cell, eigenstrain, tangent):
        assert P is not None, "solve_nonlinear(load=True) passes the load to every call"
        self.secant_calls.append((len(coef), np.shape(P), per_cell, eigenstrain))
        P = np.asarray(P, dtype=float)
        make = SL.cells(self.kind, self.dim, self.n)
        rs = []
        for k in range(len(coef)):
            load = P[k, 0] if per_cell else P[0]
            r = SL.iterate(make, law, coef[k], xi[k], load, eigenstrain, None if M is None else M[k], rows[k, :3], points,
                           rows[k, 3:] if law.n_fields else None, max_iter, tol, relax)
            if tangent:
                r.update(SL.tangent(self.kind, self.dim, self.dlaw, r, coef[k], xi[k], None if M is None else M[k], n=self.n))
            rs.append(r)
        col = lambda name, dtype=float: np.array([r[name] for r in rs], dtype=dtype)
        out = SecantResult(np.stack([r["A"] for r in rs]), np.stack([r["mean_flux"] for r in rs]), col("rounds", np.int64), col("change"),
                           col("status", np.int64), np.zeros(len(coef), np.int32))
        if tangent:
            out.tangent, out.asymmetry, out.tangent_info = np.stack([r["D"] for r in rs]), col("asymmetry"), np.zeros(len(coef), np.int32)
        return out

    def secant(self, coef, xi, law, M=None, rows=None, points=None, max_iter=50, tol=1e-10, relax=1.0, P=None, per_cell=None, eigenstrain=False):
        return self._rounds(coef, xi, law, M, rows, points, max_iter, tol, relax, P, per_cell, eigenstrain, False)

    def secant_tangent(self, coef, xi, law, tangent_plan, M=None, rows=None, points=None, max_iter=50, tol=1e-10, relax=1.0, P=None,
                       per_cell=None, eigenstrain=False):
        assert tangent_plan is self.sibling
        return self._rounds(coef, xi, law, M, rows, points, max_iter, tol, relax, P, per_cell, eigenstrain, True)


def _solver(A=None, f=40.0, nx=3, n=4, dlaw=DLAW):
    A = A or (lambda x, y: 1.0 + 0.0 * x[0] * y[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: f + x[0], mesh.create_unit_square(n, n), 0.01, quadrature_degree=3)
    h._plan = LoadSecantOraclePlan(2, n, "poisson", dlaw)
    h._tangent_plan = h._plan.sibling
    return h


def _cell_strains(h, seed=5):
    """One constant eigenstrain per macro cell, as the array [N, n_el, t] ``set_eigenstrain`` takes."""
    N, n_el = h._msh.num_cells, h._cell_mesh.num_cells
    E = 0.4 * np.random.default_rng(seed).standard_normal((N, 1, 2))
    return np.ascontiguousarray(np.broadcast_to(E, (N, n_el, 2))), E[:, 0]


@pytest.mark.parametrize("method", ["secant", "newton"])
def test_the_identity_law_with_a_load_is_solve_with_that_load(method):
    A = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * x[0]) + 0.9 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1])
    h = _solver(A, f=1.0, dlaw=IDENTITY[1])
    h.set_eigenstrain(lambda x, y: [0.3 + 0.2 * np.sin(2 * np.pi * y[0]) + 0.0 * x[0], -0.1 + 0.0 * x[0] * y[0]])
    u = h.solve().x.array.copy()
    P_eff = h.effective_polarisation.copy()
    v = h.solve_nonlinear(IDENTITY[0], load=True, method=method).x.array
    assert len(h.nonlinear_history) == 1 and h.nonlinear_history[0] <= 1e-12
    assert np.abs(v - u).max() <= 1e-12 * np.abs(u).max()
    assert np.abs(h.effective_polarisation - P_eff).max() <= 1e-12 * np.abs(P_eff).max()  # mean_flux - A_eff xi is Levin's P_eff
    assert all(c[2] is True and c[3] is True for c in h._plan.secant_calls)  # sampled per cell, the eigenstrain as it is
    assert h._linearisation_load is None and not h._nonlinear_load and h._needs_reassembly
    assert np.abs(h.solve().x.array - u).max() <= 1e-12 * np.abs(u).max()  # the next solve() is the linear one again


@pytest.mark.parametrize("method", ["secant", "newton"])
def test_every_macro_iterate_is_that_of_the_numpy_loop(method):
    """A homogeneous micro coefficient and one constant eigenstrain E_T per macro cell: the micro state of a cell is uniform, its
    elastic strain g = xi - E_T, so the secant tensor is a(|g|) I, the mean flux a g and the tangent a I - g g^T / (1 + |g|^2)^2.  The
    macro iterates are those of a loop assembled here from these closed forms through the solver's own helpers."""
    h = _solver()
    E_field, E = _cell_strains(h)
    h.set_eigenstrain(E_field)
    cells = np.arange(h._msh.num_cells)
    u = h.solve().x.array.copy()
    for k in range(1, 5):
        g = h._macro_strains(cells, u) - E
        s = 1.0 + (g**2).sum(axis=1)
        a = 0.5 + 0.5 / s
        secant = a[:, None, None] * np.eye(2)
        matrix = secant - np.einsum("cm,cn->cmn", g, g) / (s**2)[:, None, None] if method == "newton" else secant
        h._set_macro_matrix(h._local_stiffness_from_tensors(cells, matrix))
        h._linearisation_load, h._nonlinear_load = a[:, None] * g - np.einsum("cmn,cn->cm", matrix, g + E), True
        try:
            u = h.solve().x.array.copy()
        finally:
            h._linearisation_load, h._nonlinear_load = None, False
        h._needs_reassembly = True  # solve_nonlinear starts from the linear solve()
        got = h.solve_nonlinear(LAW, max_iter=k, tol=0.0, load=True, method=method, micro_tol=1e-13, micro_iter=200).x.array
        dev = np.abs(got - u).max() / np.abs(u).max()
        print(f"{method}: macro iterate {k}, deviation from the NumPy loop {dev:.3e}")
        assert dev <= 1e-10, (k, dev)
        assert len(h.nonlinear_history) == k
    assert h.nonlinear_history[0] > 1e-3  # the load and the law matter
    assert np.abs(h.effective_tensors - secant).max() <= 1e-10
    assert np.abs(h.effective_polarisation + a[:, None] * E).max() <= 1e-10  # mean_flux - A_eff xi = a g - a (g + E)


def test_newton_and_secant_agree_to_the_macro_tolerance():
    h = _solver(lambda x, y: 1.0 + 0.3 * np.sin(2 * np.pi * y[0]) + 0.1 * x[0])
    h.set_polarisation(lambda x, y: [0.5 + 0.3 * np.cos(2 * np.pi * y[1]) + x[0], 0.2 * np.sin(2 * np.pi * y[0]) + 0.0 * x[0]])
    us = h.solve_nonlinear(LAW, max_iter=80, tol=1e-11, micro_tol=1e-13, micro_iter=200, load=True).x.array.copy()
    hs = list(h.nonlinear_history)
    un = h.solve_nonlinear(LAW, max_iter=80, tol=1e-11, micro_tol=1e-13, micro_iter=200, load=True, method="newton").x.array
    dev = np.abs(un - us).max() / np.abs(us).max()
    print(f"secant {len(hs)} steps, newton {len(h.nonlinear_history)} steps, |u_newton - u_secant| = {dev:.2e} of max |u|")
    assert hs[-1] <= 1e-11 and h.nonlinear_history[-1] <= 1e-11 and dev <= 1e-8 and len(h.nonlinear_history) < len(hs)
    assert all(c[3] is False for c in h._plan.secant_calls)  # a polarisation


def test_the_runtime_errors():
    h = _solver()
    with pytest.raises(RuntimeError, match=r"set_polarisation\(\) or set_eigenstrain\(\)"):
        h.solve_nonlinear(LAW, load=True)
    h.set_polarisation(np.zeros((32, 2)))
    with pytest.raises(RuntimeError, match="polarisation.*load=True"):
        h.solve_nonlinear(LAW)
    h.set_eigenstrain(np.zeros((32, 2)))
    with pytest.raises(RuntimeError, match="polarisation.*load=True"):
        h.solve_nonlinear(LAW, method="newton")
    assert not h._plan.secant_calls


# -- two ranks over gloo -----------------------------------------------------------------------------------------------------------------
def _gloo_problem():
    h = _solver(lambda x, y: 1.0 + 0.3 * np.sin(2 * np.pi * y[0]) + 0.1 * x[0], f=30.0)
    h.set_eigenstrain(_cell_strains(h)[0])
    return h


def _gloo_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    h = _gloo_problem()
    out = {}
    for method in ("secant", "newton"):
        h._plan.secant_calls.clear()
        u = h.solve_nonlinear(LAW, max_iter=3, tol=0.0, load=True, method=method).x.array.copy()
        r = h.secant
        out[method] = {"u": u, "A": r.A_eff, "flux": r.mean_flux, "rounds": r.rounds, "status": r.status, "P": h.effective_polarisation,
                       "cells": [c[0] for c in h._plan.secant_calls], "history": h.nonlinear_history}
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_solve_nonlinear_with_a_load():
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
    for method in ("secant", "newton"):
        u = h.solve_nonlinear(LAW, max_iter=3, tol=0.0, load=True, method=method).x.array
        for r in (0, 1):
            g = got[r][method]
            assert g["cells"] == [9, 9, 9]  # every rank iterated only its 9 of the 18 cells, in each of the three macro steps
            assert np.array_equal(g["u"], u) and g["history"] == h.nonlinear_history
            for name, want in (("A", h.secant.A_eff), ("flux", h.secant.mean_flux), ("rounds", h.secant.rounds), ("status", h.secant.status),
                               ("P", h.effective_polarisation)):
                assert np.array_equal(g[name], want), name
