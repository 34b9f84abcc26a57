"""``criterion(nonlinear=True)`` and ``reconstruct(nonlinear=True)`` of the solver classes on the CPU: a stand-in plan whose
``secant`` with a tail is tests/secant_state_ref.py, in the manner of test_secant_load_hmm_host.py.  The identity law against the linear
``criterion``, a damage path whose driver read back as a state criterion IS the trial history, every error, the WARNING, and two gloo
ranks.  No GPU."""

import logging
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import secant_load_ref as SL
import secant_state_ref as SS
from hommx_amd import fem, hmm, mesh
from hommx_amd.batch import CriterionResult, SecantResult
from hommx_amd.expr import Criterion
from test_criterion_host import CriterionOraclePlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQ = "sqrt(e[0]**2 + e[1]**2)"
KAPPA = f"max(h[0], {EQ})"
N_MICRO = 4
SOFT = "c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"


def damage_law():
    return hmm.SecantLaw(f"c[0]*(1 - 0.5*(1 - exp(-{KAPPA}/0.7)))", history=[KAPPA], history_names=("kappa",))


class StateOraclePlan(CriterionOraclePlan):
    """``solve``, ``reconstruct``, ``loads`` and the linear ``criterion`` of the parents; ``secant`` -- with or without a load, a history
    and a tail -- answers with secant_state_ref / secant_load_ref, cell by cell.  Records what every call was given."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.secant_calls = []

    def secant(self, coef, xi, law, M=None, rows=None, points=None, max_iter=50, tol=1e-10, relax=1.0, history=None, P=None, per_cell=None,
               eigenstrain=False, criterion=None, crit_rows=None, crit_values=False, crit_fields=False, reconstruct=False, regions=None,
               n_regions=None):
        self.secant_calls.append(dict(n=len(coef), P=None if P is None else np.shape(P), eigenstrain=eigenstrain, tail=criterion is not None or reconstruct,
                                      history=None if history is None else np.array(history), crit_rows=None if crit_rows is None else np.array(crit_rows),
                                      limits=(max_iter, tol, relax)))
        make = SL.cells(self.kind, self.dim, self.n)
        rs = []
        for k in range(len(coef)):
            load = None if P is None else np.asarray(P, dtype=float)[k, 0] if per_cell else np.asarray(P, dtype=float)[0]
            kw = dict(M=None if M is None else M[k], x=rows[k, :3], y=points, fields=rows[k, 3:] if law.n_fields else None,
                      history=None if history is None else history[k], max_iter=max_iter, tol=tol, relax=relax)
            if criterion is not None:
                rs.append(SS.evaluate(make, law, criterion, coef[k], xi[k], load, eigenstrain, crit_fields=crit_rows[k, 3:] if criterion.n_fields else None, **kw))
            else:
                zero = np.zeros((coef.shape[1], len(xi[k])))
                rs.append(SL.iterate(make, law, coef[k], xi[k], zero if load is None else load, eigenstrain and load is not None, kw.pop("M"),
                                     kw.pop("x"), kw.pop("y"), kw.pop("fields"), **kw))
        col = lambda name, dtype=float: np.array([r[name] for r in rs], dtype=dtype)
        A, info = np.stack([r["A"] for r in rs]), np.zeros(len(coef), np.int32)
        out = SecantResult(A, np.stack([r["mean_flux"] for r in rs]), col("rounds", np.int64), col("change"), col("status", np.int64), info)
        if history is not None:
            out.history = np.stack([r["history"] for r in rs])
        if criterion is not None:
            out.criterion = CriterionResult(col("max"), col("argmax_element", np.int64), col("mean"), col("exceed_volume"), A, info,
                                            col("values") if crit_values else None, col("total_strain") if crit_fields else None,
                                            col("total_flux") if crit_fields else None)
        if reconstruct:
            assert regions is None
            out.reconstruction = self.reconstruct(np.stack([r["coef"] for r in rs]), xi, M)
        return out


def _solver(A=None, nx=2, n=N_MICRO, f=0.0):
    A = A or (lambda x, y: 1.0 + 0.3 * np.sin(2 * np.pi * y[0]) + 0.1 * x[0])
    h = hmm.PoissonHMM(mesh.create_unit_square(nx, nx), A, lambda x: f + 0.0 * x[0], mesh.create_unit_square(n, n), 0.01, quadrature_degree=3)
    h._plan = StateOraclePlan(2, n, "poisson")
    return h


def _bcs(h, scale):
    """u = scale * (x0 + x1^2 / 2) on the boundary: the load steps scale a macro gradient that differs from cell to cell."""
    V = h.function_space
    g = fem.Function(V)
    g.x.array[:] = scale * (V.mesh.geometry.x[:, 0] + 0.5 * V.mesh.geometry.x[:, 1] ** 2)
    return [fem.dirichletbc(g, hmm._box_boundary_nodes(V.mesh), V)]


# -- the identity law ---------------------------------------------------------------------------------------------------------------------
def test_after_the_identity_law_the_nonlinear_criterion_is_the_linear_one():
    h = _solver(f=30.0)
    h.set_boundary_conditions(_bcs(h, 1.0))
    h.solve_nonlinear(hmm.SecantLaw("c[0]"))
    crit = Criterion("sqrt(s[0]**2 + s[1]**2)/where(c[0] > 1.1, 2, 1) + 0.125*y[0] + x[1]", threshold=1.5)
    lin = h.criterion(crit, values=True, fields=True)
    non = h.criterion(crit, nonlinear=True, values=True, fields=True)
    for name in ("max", "mean", "exceed_volume", "values", "strain", "flux"):
        a, b = getattr(non, name), getattr(lin, name)
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), name
    assert np.array_equal(non.argmax_element, lin.argmax_element) and np.array_equal(non.cells, lin.cells)
    assert non.secant is not None and not non.secant.status.any() and np.array_equal(non.secant.rounds, np.ones(len(non.cells), dtype=np.int64))
    assert non.secant.criterion is None and lin.secant is None
    rec, nrec = h.reconstruct(), h.reconstruct(nonlinear=True)
    for name in ("mean_strain", "mean_flux", "energy", "max_flux"):
        assert np.abs(getattr(nrec, name) - getattr(rec, name)).max() <= 1e-12 * max(1.0, np.abs(getattr(rec, name)).max()), name
    assert np.array_equal(nrec.cells, rec.cells) and nrec.secant is not None and nrec.strain is None


def test_cells_chunks_and_field_values_reach_the_plan():
    h = _solver(f=30.0)
    n = h._msh.num_cells
    h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=3, tol=0.0, micro_iter=7, micro_tol=1e-9, relax=0.75)
    crit = Criterion("sqrt(s[0]**2 + s[1]**2)/f[0] + b[0] - c[0]", fields=("strength",))
    strength = 1.0 + np.arange(n) / n
    full = h.criterion(crit, nonlinear=True, field_values=strength, values=True)
    h._plan.secant_calls.clear()
    cells = np.array([5, 1, 6])
    part = h.criterion(crit, nonlinear=True, field_values=strength, values=True, cells=cells, chunk_cells=2)
    calls = h._plan.secant_calls
    assert [c["n"] for c in calls] == [2, 1] and all(c["tail"] and c["limits"] == (7, 1e-9, 0.75) for c in calls)
    assert np.array_equal(np.concatenate([c["crit_rows"][:, 3] for c in calls]), strength[cells])  # the criterion's own rows, cell by cell
    assert np.array_equal(part.cells, cells) and np.array_equal(part.values, full.values[cells]) and np.array_equal(part.max, full.max[cells])
    assert np.array_equal(part.secant.rounds, full.secant.rounds[cells]) and np.array_equal(part.secant.cells, cells)
    flux = h.criterion(Criterion("s[0]"), nonlinear=True, fields=True).flux
    gap = full.values - np.sqrt((flux ** 2).sum(axis=2)) / strength[:, None]  # b[0] - c[0]: the law softens, and not where nothing strains
    assert (gap >= -1e-14).all() and (gap > 1e-3).any()
    with pytest.raises(RuntimeError, match="field_values"):
        h.criterion(crit, nonlinear=True)
    u = h._u.x.array.copy()
    assert np.array_equal(h.criterion(crit, u, nonlinear=True, field_values=strength).max, full.max)  # the default u is the last result


# -- damage over load steps ----------------------------------------------------------------------------------------------------------------
def test_the_driver_of_the_damage_read_as_a_state_criterion_is_the_trial_history():
    """Load, unload, reload.  After each converged step one more macro step from its solution u runs the micro iteration AT u, so
    ``history_trial`` belongs to u and ``criterion(driver, u, nonlinear=True)`` re-runs the same rounds on the same numbers: the law is
    made of exactly rounded operations up to ``exp``, which the driver does not contain, so the values are the trial history, bit for
    bit -- before and after the commit, which is what the kept reference to the starting history is for."""
    h, law = _solver(), damage_law()
    driver = Criterion(KAPPA, history=1)
    u, seen = None, []
    for scale in (1.0, 0.5, 1.5):
        h.set_boundary_conditions(_bcs(h, scale))
        u = h.solve_nonlinear(law, max_iter=40, tol=1e-10, micro_tol=1e-12, u0=u).x.array.copy()
        assert not h.secant.status.any() and h.nonlinear_history[-1] <= 1e-10
        h.solve_nonlinear(law, max_iter=1, micro_tol=1e-12, u0=u)  # the micro iteration at u itself; no commit in between: the same start
        start = None if h.history is None else h.history.copy()
        trial = h.history_trial.copy()
        before = h.criterion(driver, u, nonlinear=True, values=True)
        assert np.array_equal(before.values, trial[:, :, 0]), scale
        assert np.array_equal(before.max, trial[:, :, 0].max(axis=1)) and not before.secant.status.any()
        h.commit_history()
        after = h.criterion(driver, u, nonlinear=True, values=True)
        assert np.array_equal(after.values, trial[:, :, 0]), scale  # still the state the step ended in, not one step further
        assert np.array_equal(h.history, trial) and (start is None or np.array_equal(h._nonlinear_state["history"], start))
        seen.append(trial)
    assert np.array_equal(seen[1], seen[0]) and (seen[2] > seen[0]).mean() > 0.9  # unloading keeps it, reloading grows it
    # the failed volume fraction of the matrix and the mean stress of a phase are one call each
    frac = h.criterion(Criterion(f"where(b[0] > 1.2, 0, {KAPPA})", history=1, threshold=0.5), u, nonlinear=True)
    assert frac.exceed_volume.shape == (h._msh.num_cells,) and (frac.exceed_volume <= 1).all() and frac.exceed_volume.max() > 0
    soft = h.criterion(Criterion("c[0]/b[0]"), u, nonlinear=True, values=True)  # an undeclared criterion on the row of a law with history
    assert (soft.values < 1).all() and (soft.values > 0.5).all()


# -- errors -----------------------------------------------------------------------------------------------------------------------------
def test_every_error_names_what_to_do():
    h = _solver(f=30.0)
    crit, state = Criterion("s[0]"), Criterion("s[0]/b[0]")
    with pytest.raises(RuntimeError, match=r"criterion\(nonlinear=True\).*call solve_nonlinear\(\) first"):
        h.criterion(crit, nonlinear=True)
    with pytest.raises(RuntimeError, match=r"reconstruct\(nonlinear=True\).*call solve_nonlinear\(\) first"):
        h.reconstruct(nonlinear=True)
    h.solve()
    with pytest.raises(RuntimeError, match="solve_nonlinear"):  # a linear solve is no nonlinear state
        h.criterion(crit, nonlinear=True)
    with pytest.raises(ValueError, match=r"reads b\[0\], the nonlinear state: pass nonlinear=True"):
        h.criterion(state)
    with pytest.raises(ValueError, match=r"reads h\[0\], the nonlinear state: pass nonlinear=True"):
        h.criterion(Criterion("h[0]", history=1))
    h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=2, tol=0.0)
    for load in (True, False):
        with pytest.raises(ValueError, match=r"takes no load=.*part of its state"):
            h.criterion(crit, nonlinear=True, load=load)
    with pytest.raises(ValueError, match=r"declares history=1; the law of solve_nonlinear has 0"):
        h.criterion(Criterion("h[0]", history=1), nonlinear=True)
    with pytest.raises(ValueError, match=r"criterion\(crit, nonlinear=True, fields=True\)"):
        h.reconstruct(nonlinear=True, fields=True)
    assert h.criterion(state, nonlinear=True).max.shape == (h._msh.num_cells,)
    # a solver that ran with its load
    h.set_eigenstrain(lambda x, y: [0.3 + 0.2 * np.sin(2 * np.pi * y[0]) + 0.0 * x[0], -0.1 + 0.0 * x[0] * y[0]])
    h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=2, tol=0.0, load=True)
    with pytest.raises(RuntimeError, match=r"load=True.*no load term.*criterion\(crit, nonlinear=True, fields=True\)"):
        h.reconstruct(nonlinear=True)
    h._plan.secant_calls.clear()
    loaded = h.criterion(crit, nonlinear=True, fields=True)
    assert all(c["P"] is not None and c["eigenstrain"] for c in h._plan.secant_calls)  # the load of the run, the eigenstrain as it is
    assert loaded.flux.shape == (h._msh.num_cells, 2 * N_MICRO**2, 2)
    periodic = hmm.PoissonPeriodicHMM(mesh.create_unit_square(2, 2), lambda y: 1.0 + 0.0 * y[0], lambda x: 1.0 + 0.0 * x[0],
                                      mesh.create_unit_square(4, 4), 0.01)
    for call in (lambda: periodic.criterion(crit, nonlinear=True), lambda: periodic.reconstruct(nonlinear=True), periodic.solve_nonlinear):
        with pytest.raises(RuntimeError, match="PoissonHMM"):
            call()


def test_one_warning_counts_the_statuses(caplog):
    h = _solver(lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]) + 0.0 * x[0], f=30.0)
    crit = Criterion("s[0]")
    h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=30, tol=1e-9)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        r = h.criterion(crit, nonlinear=True)
    assert not caplog.records and not r.secant.status.any()
    with caplog.at_level(logging.WARNING):
        h.solve_nonlinear(hmm.SecantLaw(SOFT), max_iter=2, tol=0.0, micro_iter=2, micro_tol=0.0)  # two rounds at tol 0 do not settle a cell
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        r = h.criterion(crit, nonlinear=True, chunk_cells=3)
    warnings = [x for x in caplog.records if x.levelno == logging.WARNING]
    stopped = int((r.secant.status == 1).sum())  # the cells without a macro gradient settle at once
    assert len(warnings) == 1 and stopped > 0 and set(r.secant.status.tolist()) == {0, 1}  # one WARNING for the three chunks together
    text = warnings[0].getMessage()
    assert "criterion(nonlinear=True)" in text and f"0: {h._msh.num_cells - stopped}, 1: {stopped}" in text


# -- two ranks over gloo -----------------------------------------------------------------------------------------------------------------
def _gloo_steps(h):
    law, driver = damage_law(), Criterion(KAPPA, history=1)
    h.set_boundary_conditions(_bcs(h, 1.0))
    u = h.solve_nonlinear(law, max_iter=3, tol=0.0).x.array.copy()
    h.solve_nonlinear(law, max_iter=1, u0=u)
    return u, driver


def _gloo_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    h = _solver()
    u, driver = _gloo_steps(h)
    own = h.history_cells
    r = h.criterion(driver, u, nonlinear=True, values=True, cells=own)  # this rank alone, for its own cells: no collective
    refused = ""
    try:
        h.criterion(driver, u, nonlinear=True)  # every cell: the other rank's history is not here
    except ValueError as e:
        refused = str(e)
    blind = h.criterion(Criterion("c[0]/b[0]"), u, nonlinear=True, cells=own[:1])
    q.put((rank, {"cells": own, "values": r.values, "trial": h.history_trial, "refused": refused, "max": r.max, "blind": blind.max}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_evaluate_the_cells_whose_history_they_hold():
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
    h = _solver()
    u, driver = _gloo_steps(h)
    want = h.criterion(driver, u, nonlinear=True, values=True)
    for r in (0, 1):
        block = np.arange(4 * r, 4 * (r + 1))
        g = got[r]
        assert np.array_equal(g["cells"], block)
        assert np.array_equal(g["values"], g["trial"][:, :, 0]) and np.array_equal(g["values"], want.values[block])
        assert np.array_equal(g["max"], want.max[block])
        assert "history_cells" in g["refused"] and f"cell {4 * (1 - r)} is not among them" in g["refused"]
        assert g["blind"].shape == (1,)
