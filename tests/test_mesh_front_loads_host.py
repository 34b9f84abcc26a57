"""The load solve of the frontal mesh route by substitution on its pivot columns ("load solves"), host side: the record and
the two passes k_mesh_front_rhs implements, stated in NumPy (tests/mesh_front_rhs_ref.py), against loads_ref's sparse solve for every
kind on the meshes of the GPU tests; the flag and its way from the solver classes to the descriptor (CPU only).

Bound: 1e-11 relative to the largest corrector entry, the bar tests/test_fused_rhs_host.py holds the same kind of restatement to."""

import functools
import os
import re

import numpy as np
import pytest

import loads_ref as L
import mesh_front_rhs_ref as R
from hommx_amd import hmm, mesh as Mm, workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("poisson", "poisson_matrix", "elasticity", "elasticity_voigt")
# the two meshes of tests/stream_order_gpu.mesh, and the smallest: 9 nodes, 8 steps, bs = 2 for elasticity
MESHES = {"square_9x7": lambda: W.jittered_unit_square(9, 7), "cube_3x4x3": lambda: W.jittered_unit_cube(3, 4, 3),
          "square_3x3": lambda: Mm.create_unit_square(3, 3)}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return MESHES[name]()


def _err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@functools.lru_cache(maxsize=None)
def _cell(name, kind, with_M):
    msh = _mesh(name)
    dim = msh.topology.dim
    rng = np.random.default_rng(sorted(MESHES).index(name) * 100 + KINDS.index(kind) * 10 + with_M)
    coef = L.random_coef(kind, dim, msh.num_cells, rng)
    cell = L.on_mesh(msh, kind, coef, L.random_M(dim, rng) if with_M else None)
    P = L.random_loads(rng, cell.t, cell.n_el, cell.t)
    return cell, P, cell.solve(P), rng.permutation(cell.nn)


@pytest.mark.parametrize("with_M", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MESHES))
def test_passes_reproduce_the_reference(name, kind, with_M):
    """t loads at once, in the natural node order and in a random one (another pinned node, other fronts)."""
    cell, P, want, perm = _cell(name, kind, with_M)
    K = R.dense_stiffness(cell)
    for order in (np.arange(cell.nn), perm):
        record = R.factor(K, order, cell.bs)
        assert len(record) == (cell.nn - 1) * cell.bs
        assert R.same_node_rows_cleared(record, cell.bs) == (cell.nn - 1) * cell.bs * (cell.bs - 1) // 2
        err = _err(R.correctors(record, want["f"], order, cell.bs), want["chi"])
        print(name, kind, with_M, err)
        assert err < 1e-11


@pytest.mark.parametrize("kind", ["poisson", "elasticity"])
def test_canonical_loads_give_the_canonical_correctors(kind):
    """P = material(coef) e_m: the border rows of the elimination carry exactly this forward pass."""
    cell, _, _, perm = _cell("square_3x3", kind, True)
    f = cell.load_vector(np.transpose(cell.V, (2, 0, 1)))
    got = R.correctors(R.factor(R.dense_stiffness(cell), perm, cell.bs), f, perm, cell.bs)
    assert _err(got, cell.chi_canon) < 1e-11


# -- plumbing ------------------------------------------------------------------------------------------------------------------------------
def test_flag_equals_the_header():
    from hommx_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "hommx_hip.h")).read()
    values = {name: int(v) for name, v in re.findall(r"#define\s+HOMMX_MESH_FLAG_(\w+)\s+(\d+)", hdr)}
    assert values == {"TREE": _lib.MESH_FLAG_TREE, "LOADS": _lib.MESH_FLAG_LOADS} and _lib.MESH_FLAG_LOADS == 2


class _Recorder:
    """Stands where hmm.py looks MicroCellPlan up: records how a plan was asked for."""

    calls: list = []

    def __init__(self, *args, **kw):
        type(self).calls.append(("structured", args, kw))
        self.kind = args[2]

    @classmethod
    def from_mesh(cls, msh, kind, **kw):
        cls.calls.append(("from_mesh", (msh, kind), kw))
        self = object.__new__(cls)
        self.kind = kind
        return self


@pytest.mark.parametrize("which", ["unstructured", "structured"])
def test_solver_classes_ask_for_the_load_solve(which, monkeypatch):
    monkeypatch.setattr(hmm, "MicroCellPlan", _Recorder)
    monkeypatch.setattr(_Recorder, "calls", [])
    micro = W.jittered_unit_square(9, 7) if which == "unstructured" else Mm.create_unit_square(4, 4)
    h = hmm.PoissonHMM(Mm.create_unit_square(2, 2), lambda x, y: 1.0 + 0 * y[0], lambda x: 1.0 + x[0], micro, 0.01, quadrature_degree=0, device=0)
    e = hmm.LinearElasticityHMM(Mm.create_unit_square(2, 2), lambda x, y: hmm.Lame(1.0 + 0 * y[0], 1.0 + 0 * y[0]), lambda x: np.zeros(2), micro,
                                0.01, quadrature_degree=0, device=0)
    h._ensure_plan("poisson")
    e._ensure_plan("elasticity")
    assert len(_Recorder.calls) == 2
    for how, _, kw in _Recorder.calls:
        if which == "unstructured":
            assert how == "from_mesh" and kw.get("load_solve") is True and kw.get("route") is None
        else:
            assert how == "structured"  # from_mesh is never called


def test_from_mesh_sets_the_flag(monkeypatch):
    """load_solve -> HOMMX_MESH_FLAG_LOADS in the descriptor, beside the route's flag; no device is touched (mesh_desc is patched)."""
    from hommx_amd import _lib, batch

    seen = []

    def fake_desc(msh, kind, device, order, constraint, flags=0):
        seen.append(flags)
        raise KeyboardInterrupt  # stop before the library is asked for a plan

    monkeypatch.setattr(batch, "mesh_desc", fake_desc)
    for kw, want in (({}, 0), ({"load_solve": True}, _lib.MESH_FLAG_LOADS), ({"route": "tree", "load_solve": True}, _lib.MESH_FLAG_TREE | _lib.MESH_FLAG_LOADS),
                     ({"route": "front", "load_solve": False}, 0)):
        with pytest.raises(KeyboardInterrupt):
            batch.MicroCellPlan.from_mesh(None, "poisson", **kw)
        assert seen[-1] == want
