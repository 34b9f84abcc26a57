"""User-supplied polarisation loads on the CPU: the NumPy / SciPy reference checked against ``periodic_fem.solve_cell`` and
its own identities before anything leans on it, the argument checks of hommx_loads_source[_device] (they run before any device is
touched), the solver classes on oracle-backed stub plans (the shift identity), and a two-rank gloo run (no GPU needed)."""

import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import loads_ref as L
import periodic_fem as PF
from hommx_amd import _lib, fem, hmm, mesh, workloads as W
from hommx_amd.batch import LoadResponse
from test_reconstruct_host import ReconOraclePlan
from test_reconstruct_source_host import _fake_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")
MESHES = {"square": lambda: mesh.create_unit_square(6, 6), "jittered": lambda: W.jittered_unit_square(7, 5),
          "cube": lambda: mesh.create_unit_cube(3, 3, 3)}


def _err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


# -- 1. the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MESHES))
def test_reference_checks_itself(name, kind):
    msh = MESHES[name]()
    dim = msh.topology.dim
    rng = np.random.default_rng(list(MESHES).index(name) + 10 * KINDS.index(kind))
    coef = L.random_coef(kind, dim, msh.num_cells, rng)
    M = L.random_M(dim, rng)
    ref = L.on_mesh(msh, kind, coef, M)
    P = L.random_loads(rng, ref.t, ref.n_el, ref.t)
    r = ref.solve(P)
    assert _err(r["P_eff"], ref.levin(P)) < 1e-11  # the direct mean total flux is the Levin value
    assert _err(r["energy"], r["energy_P"]) < 1e-11 and _err(r["energy"], r["energy"].T) < 1e-11  # both forms of the energy
    assert np.abs(r["f"].reshape(len(P), ref.nn, ref.bs).sum(axis=1)).max() < 1e-12 * np.abs(r["f"]).max()  # mean-free loads
    # P = material(coef) e_m is the canonical problem of periodic_fem.solve_cell (its own assembly, on the full Hooke tensor)
    A, chi, node = PF.solve_cell(msh, kind, coef, M)
    assert np.array_equal(node, PF.periodic_map(msh.geometry.x, dim)[0])
    assert _err(ref.chi_canon, chi) < 1e-11 and _err(ref.A, A) < 1e-11
    canon = ref.solve(np.transpose(ref.V, (2, 0, 1)))
    assert _err(canon["energy"], ref.C0 - A) < 1e-11


def test_reference_structured_numbering_matches_the_mesh():
    rng = np.random.default_rng(4)
    coef = L.random_coef("elasticity", 2, 2 * 25, rng)
    P = L.random_loads(rng, 2, 50, 3)
    a, b = L.structured("elasticity", 2, 5, coef).solve(P), L.on_mesh(mesh.create_unit_square(5, 5), "elasticity", coef).solve(P)
    assert _err(a["q"], b["q"]) < 1e-11 and _err(a["P_eff"], b["P_eff"]) < 1e-11


# -- 2. C ABI argument checks -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_loads_source_device if device_entry else lib.hommx_loads_source
    tail = (None,) if device_entry else ()

    def call(plan, src, args, n_cells=1):
        rc = fn(plan, n_cells, src, None, None if args is None else ctypes.byref(args), *tail)
        return rc, lib.hommx_last_error().decode()

    def args(**kw):
        return _lib.LoadArgs(**dict(dict(n_loads=1, per_cell=0, P=p, P_eff=p), **kw))

    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    for kind, t in ((_lib.KIND_POISSON_SCALAR, 2), (_lib.KIND_ELASTICITY_ISO, 3)):
        fake = _fake_plan(kind)
        plan = ctypes.addressof(fake)
        assert lib.hommx_plan_kind(plan) == kind
        rc, msg = call(None, sampled, args())
        assert rc == -1 and "null plan" in msg
        assert call(None, sampled, args(), n_cells=0)[0] == -1  # a null plan, even when empty
        rc, msg = call(plan, sampled, args(), n_cells=-1)
        assert rc == -1 and "negative n_cells" in msg
        assert call(plan, None, None, n_cells=0)[0] == 0  # an empty batch reads nothing
        rc, msg = call(plan, sampled, None)
        assert rc == -1 and msg == "null arguments"
        for nl in (0, t + 1, -3):
            rc, msg = call(plan, sampled, args(n_loads=nl))
            assert rc == -1 and msg == f"n_loads must be 1 .. {t} (the tensor size of the plan), got {nl}"
        for kw in ({"P": None}, {"P_eff": None}):
            rc, msg = call(plan, sampled, args(**kw))
            assert rc == -1 and msg == "null P / P_eff"
        for kw in ({"strain": p}, {"flux": p}):
            rc, msg = call(plan, sampled, args(**kw))
            assert rc == -1 and msg == "strain and flux: both or neither"
        rc, msg = call(plan, None, args())
        assert rc == -1 and "null source" in msg
        rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=7, coef=p)), args())
        assert rc == -1 and "unknown coefficient form 7" in msg
        rc, msg = call(plan, ctypes.byref(_lib.CoefSource(form=_lib.COEF_TWO_PHASE, mask=p)), args())
        assert rc == -1 and "null mask / values" in msg
    if device_entry:
        rc, msg = call(plan, sampled, args(), n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg


# -- 3. solver classes on an oracle-backed stub plan -----------------------------------------------------------------------------------------
class LoadOraclePlan(ReconOraclePlan):
    """Answers loads() with the reference's Levin value; records what it was given."""

    def __init__(self, dim, n, kind):
        super().__init__(dim, n, kind)
        self.load_calls = []

    def loads(self, coef, P, M=None, per_cell=None, response=False, fields=False, return_correctors=False):
        self.load_calls.append((np.shape(coef), np.shape(P), per_cell, response))
        cells = [L.structured(self.kind, self.dim, self.n, coef[k], None if M is None else M[k]) for k in range(len(coef))]
        P_eff = np.stack([c.levin(P[k] if per_cell else P) for k, c in enumerate(cells)])
        r = LoadResponse(P_eff, np.stack([c.A for c in cells]), np.zeros(len(coef), np.int32))
        if response:
            rs = [c.solve(P[k] if per_cell else P) for k, c in enumerate(cells)]
            r.energy, r.mean_flux = np.stack([x["energy"] for x in rs]), np.stack([x["P_eff"] for x in rs])
            r.max_flux, r.argmax_element = np.stack([x["max_flux"] for x in rs]), np.stack([x["argmax_element"] for x in rs])
            if fields:
                r.strain, r.flux = np.stack([x["eps"] for x in rs]), np.stack([x["q"] for x in rs])
        return r


E0 = {"poisson": np.array([0.7, -0.4]), "elasticity": np.array([[0.3, 0.25], [0.25, -0.6]])}


def _solver(kind):
    if kind == "poisson":
        A = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * x[0]) + 0.9 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1])
        h = hmm.PoissonHMM(mesh.create_unit_square(6, 6), A, lambda x: 1.0 + x[0], mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
        P = lambda x, y: [A(x, y) * E0[kind][0], A(x, y) * E0[kind][1]]  # material(A) E0
        u0 = lambda X: E0[kind] @ X[:2]
        g = lambda X: 0.3 * X[0] * X[1]
    else:
        lam = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]) + 0.2 * x[1]
        mu = lambda x, y: 0.6 + 0.3 * np.cos(2 * np.pi * y[1]) + 0.1 * x[0]
        h = hmm.LinearElasticityHMM(mesh.create_unit_square(4, 4), lambda x, y: hmm.Lame(lam(x, y), mu(x, y)), lambda x: np.array([0.0, -1.0]),
                                    mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
        E = E0[kind]
        tr = E[0, 0] + E[1, 1]
        P = lambda x, y: [lam(x, y) * tr + 2 * mu(x, y) * E[0, 0], lam(x, y) * tr + 2 * mu(x, y) * E[1, 1], 2 * mu(x, y) * E[0, 1]]  # C : E0
        u0 = lambda X: E @ X[:2]
        g = lambda X: np.stack([0.1 * X[1] ** 2, 0.2 * X[0]])
    h._plan = LoadOraclePlan(2, 4, kind)
    return h, P, u0, g


def _solve(h, data):
    V = h.function_space
    bnd = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1) | np.isclose(x[1], 0) | np.isclose(x[1], 1))
    gf = fem.Function(V)
    gf.interpolate(data)
    h.set_boundary_conditions(fem.dirichletbc(gf, bnd, V))
    return h.solve().x.array.copy()


@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_shift_identity(kind):
    """P = material(A) E0 is the load of the macro strain E0: with u0 the interpolant of E0 x, solve() with the polarisation and data g
    equals solve() without it and data g + u0, minus u0."""
    h, P, u0, g = _solver(kind)
    plain = _solve(h, g)
    assert h.effective_polarisation is None and not h._plan.load_calls
    shifted = _solve(h, lambda X: g(X) + u0(X))
    h.set_polarisation(P)
    with_P = _solve(h, g)
    N, t, n_el = h._msh.num_cells, h._tensor_size(), 32
    assert h._plan.load_calls == [((N, n_el) + (() if kind == "poisson" else (2,)), (N, 1, n_el, t), True, False)]
    w = fem.Function(h.function_space)
    w.interpolate(u0)
    err = _err(with_P, shifted - w.x.array)
    print(kind, "shift identity", err)
    assert err < 1e-9
    assert _err(with_P, plain) > 1e-3  # the polarisation does something
    voigt = E0[kind] if kind == "poisson" else np.array([E0[kind][0, 0], E0[kind][1, 1], 2 * E0[kind][0, 1]])
    assert h.effective_polarisation.shape == (N, t)
    assert _err(h.effective_polarisation, np.einsum("cmn,n->cm", h.effective_tensors, voigt)) < 1e-10  # P_eff = A_H E0
    # the same polarisation as element means per macro cell
    means = h._polarisation_loads(np.arange(N))[0][:, 0]
    h.set_polarisation(means)
    assert np.array_equal(_solve(h, g), with_P)
    # None restores the plain solve, bit for bit
    h.set_polarisation(None)
    assert np.array_equal(_solve(h, g), plain) and h.effective_polarisation is None


@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_zero_polarisation_and_shapes(kind):
    h, P, u0, g = _solver(kind)
    plain = _solve(h, g)
    t = h._tensor_size()
    h.set_polarisation(np.zeros((32, t)))  # shared by all macro cells
    assert np.array_equal(_solve(h, g), plain)
    assert h._plan.load_calls[-1][1:3] == ((1, 32, t), False) and not h.effective_polarisation.any()
    h.set_polarisation(lambda x, y: [0.0 * y[0]] * t)
    assert np.array_equal(_solve(h, g), plain)
    for bad in (np.zeros((31, t)), np.zeros((32, t + 1)), np.zeros((5, 32, t)), np.zeros(32)):
        with pytest.raises(ValueError, match="P has shape"):
            h.set_polarisation(bad)
    h.set_polarisation(lambda x, y: [0.0 * y[0]] * (t + 1))
    with pytest.raises(ValueError, match="must return"):
        h.solve()
    h.set_polarisation(None)
    with pytest.raises(RuntimeError, match="set_polarisation"):
        h.load_response()


def test_load_response_wraps_the_plan():
    h, P, u0, g = _solver("poisson")
    h.set_polarisation(P)
    r = h.load_response(cells=[5, 2, 11], fields=True, chunk_cells=2)
    assert [c[0][0] for c in h._plan.load_calls] == [2, 1] and all(c[3] for c in h._plan.load_calls)
    assert np.array_equal(r.cells, [5, 2, 11]) and r.P_eff.shape == (3, 1, 2) and r.flux.shape == (3, 1, 32, 2) and r.correctors is None
    assert _err(r.mean_flux, r.P_eff) < 1e-11
    full = h.load_response()
    # (72 cells are sampled in one broadcast call, two cells one by one: the element means differ in the last bits)
    assert _err(full.P_eff[[5, 2, 11]], r.P_eff) < 1e-12 and _err(full.energy[[5, 2, 11]], r.energy) < 1e-12


# -- 4. two ranks over gloo ------------------------------------------------------------------------------------------------------------------
class _FailingPlan(LoadOraclePlan):
    def loads(self, *a, **kw):
        raise ValueError("this rank's loads fail")


def _gloo_problem(plan):
    A = lambda x, y: 0.33 + 0.15 * (np.sin(2 * np.pi * x[0]) + np.sin(2 * np.pi * y[0]))
    h = hmm.PoissonHMM(mesh.create_unit_square(3, 3), A, lambda x: 1.0 + x[0], mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
    h.set_polarisation(lambda x, y: [A(x, y) * (1.0 + x[1]), 0.5 * np.cos(2 * np.pi * y[1]) + 0.0 * x[0]])
    h._plan = plan
    return h


def _gloo_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch.distributed as dist

    from hommx_amd.dist import ShardFailure

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    plan = LoadOraclePlan(2, 4, "poisson")
    h = _gloo_problem(plan)
    u = h.solve().x.array.copy()
    out = {"u": u, "P_eff": h.effective_polarisation.copy(), "cells": [c[0][0] for c in plan.load_calls]}
    try:
        _gloo_problem(_FailingPlan(2, 4, "poisson") if rank == 1 else LoadOraclePlan(2, 4, "poisson")).solve()
        out["failure"] = "returned"
    except ValueError as exc:
        out["failure"] = "own:" + str(exc)
    except ShardFailure as exc:
        out["failure"] = "peer:" + str(exc)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_polarisation():
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
    h = _gloo_problem(LoadOraclePlan(2, 4, "poisson"))
    u = h.solve().x.array
    for r in (0, 1):
        assert got[r]["cells"] == [9]  # every rank sampled and solved only its 9 of the 18 cells
        assert np.array_equal(got[r]["u"], u) and np.array_equal(got[r]["P_eff"], h.effective_polarisation)
    assert got[1]["failure"] == "own:this rank's loads fail"
    assert got[0]["failure"].startswith("peer:") and "rank(s) [1]" in got[0]["failure"]
