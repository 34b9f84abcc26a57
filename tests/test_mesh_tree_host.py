"""The tree route's symbolic phase (hommx_mesh_analyze_tree, csrc/mesh_tree.hip) on the host: partition, separator property, tree shape,
the flop model recounted in NumPy.  No GPU."""

import numpy as np
import pytest

from hommx_amd import _lib, fem, workloads as W
from hommx_amd.batch import mesh_analyze, mesh_analyze_tree, mesh_desc
from hommx_amd.cell_problem import create_periodic_boundary_conditions

CASES = [
    ("square56_elasticity", lambda: W.jittered_unit_square(56, 56), "elasticity"),
    ("cube8_elasticity", lambda: W.jittered_unit_cube(8, 8, 8), "elasticity"),
]


def _edges(msh):
    mpc = create_periodic_boundary_conditions(fem.FunctionSpace(msh, 1))
    en = np.asarray(mpc.to_periodic)[np.asarray(msh.cells)]
    nv = en.shape[1]
    e = np.concatenate([en[:, [a, b]] for a in range(nv) for b in range(nv) if a < b])
    return np.unique(np.sort(e, axis=1), axis=0), int(mpc.num_independent)


def _ancestors(parent):
    anc = [set() for _ in parent]
    for k in range(len(parent)):
        p = parent[k]
        while p >= 0:
            anc[k].add(int(p))
            p = parent[p]
    return anc


def test_wide_mesh_is_the_one_the_frontal_analysis_refuses():
    with pytest.raises(_lib.HommxLibraryError, match="HOMMX_MESH_MAX_FRONT"):
        mesh_analyze(W.jittered_unit_square(56, 56), "elasticity")
    r = mesh_analyze_tree(W.jittered_unit_square(56, 56), "elasticity")
    assert r["n_fronts"] > 1 and r["flops_per_solve"] > 0


@pytest.mark.parametrize("name,make,kind", CASES, ids=[c[0] for c in CASES])
def test_partition_separators_and_shape(name, make, kind):
    msh = make()
    r = mesh_analyze_tree(msh, kind)
    sn, parent = r["supernode_of_node"], r["parent"]
    edges, nn = _edges(msh)
    nf = r["n_fronts"]
    # partition: every node in exactly one supernode, every supernode non-empty
    assert sn.shape == (nn,) and sn.min() >= 0 and sn.max() < nf
    assert np.all(np.bincount(sn, minlength=nf) > 0)
    # tree shape: parents after their children, the root last, at most two children, one root
    assert parent.shape == (nf,) and parent[-1] == -1 and np.all(parent[:-1] > np.arange(nf - 1))
    assert np.bincount(parent[:-1], minlength=nf).max() <= 2
    # separator property: the supernodes of the two ends of every edge lie on one root path
    anc = _ancestors(parent)
    a, b = sn[edges[:, 0]], sn[edges[:, 1]]
    ok = [(x == y) or (y in anc[x]) or (x in anc[y]) for x, y in zip(a.tolist(), b.tolist())]
    assert all(ok)
    # the gauge (the root's node of highest elimination rank, i.e. of highest id) is in the root
    root_nodes = np.nonzero(sn == nf - 1)[0]
    assert root_nodes.size > 0 and sn[root_nodes.max()] == nf - 1
    bs = 1 if kind.startswith("poisson") else msh.topology.dim
    assert r["max_front"] % bs == 0 and r["max_front"] >= bs * np.bincount(sn).max()


def _round_up(v, m):
    return (v + m - 1) // m * m


def _mf_model(sn, parent, edges, nn, bs, stage=192, front_max_t=21):
    """Recount of the multifrontal flop model (multifrontal.hip, mf_plan_build) from the tree alone."""
    nf = len(parent)
    nodes = [np.nonzero(sn == k)[0] for k in range(nf)]
    adj = [set() for _ in range(nn)]
    for u, v in edges.tolist():
        adj[u].add(v)
        adj[v].add(u)
    children = [[] for _ in range(nf)]
    for k in range(nf - 1):
        children[parent[k]].append(k)
    bnd, height = [None] * nf, [0] * nf
    for k in range(nf):  # symbolic elimination: coupled nodes and the children's boundaries, owned by a later supernode
        cand = set()
        for v in nodes[k]:
            cand |= adj[v]
        for c in children[k]:
            cand |= bnd[c]
            height[k] = max(height[k], height[c] + 1)
        bnd[k] = {v for v in cand if sn[v] > k}
    groups = {}
    for k in range(nf):
        groups.setdefault((height[k], len(nodes[k]), len(bnd[k])), []).append(k)
    flops = 0.0
    for (h, ns, nr), mem in groups.items():
        sp, rb = _round_up(ns * bs, 32), nr * bs
        rp = _round_up(rb + 8, 16)
        L = sp + rp
        s16 = _round_up(ns * bs, 16)
        T = (s16 + _round_up(rb + 8, 16)) // 16
        P = s16 // 16
        ntiles, R0, nreg = T * (T + 1) // 2, 0, T * (T + 1) // 2
        while nreg > 192:
            nreg -= T - R0
            R0 += 1
        front = T <= front_max_t and R0 <= 2 and R0 <= P and mem[0] != nf - 1 and h < height[nf - 1]
        if front:
            f = sum(2.0 * 16**3 + 8192.0 * ((T - 1 - p) + (T - 1 - p) * (T - p) / 2) for p in range(P))
        else:
            nst = 1 if (stage <= 0 or sp < 2 * stage - 64) else (sp + stage - 1) // stage
            f, off = float(sp) * rp * rp, 0
            for i in range(nst):
                base, extra = (sp // 32) // nst, (sp // 32) % nst
                si = 32 * (base + (1 if i < extra else 0))
                below, rem = L - (off + si), sp - (off + si)
                f += si**3 + 2.0 * si * si * below + 2.0 * below * rem * si
                off += si
        flops += len(mem) * f
    return flops, len(groups)


@pytest.mark.parametrize("kind,make", [("elasticity", lambda: W.jittered_unit_cube(5, 5, 6, seed=3)),
                                       ("poisson", lambda: W.jittered_unit_square(30, 26, seed=1))])
def test_flop_model_recount(kind, make, monkeypatch):
    for k in ("HOMMX_MF_STAGE", "HOMMX_MF_FRONT", "HOMMX_MF_LEAF", "HOMMX_MF_SPLIT_DEPTH"):
        monkeypatch.delenv(k, raising=False)
    msh = make()
    r = mesh_analyze_tree(msh, kind)
    edges, nn = _edges(msh)
    bs = 1 if kind.startswith("poisson") else msh.topology.dim
    flops, ng = _mf_model(r["supernode_of_node"], r["parent"], edges, nn, bs)
    assert ng == r["n_groups"]
    assert flops == pytest.approx(r["flops_per_solve"], rel=1e-12)


def test_analysis_validates_like_the_frontal_one():
    msh = W.jittered_unit_square(6, 6)
    desc, keep = mesh_desc(msh, "poisson")
    keep["el_x"] *= 1.01
    lib = _lib.load()
    assert lib.hommx_mesh_analyze_tree(desc, None, None, None, None, None, None) == -1
    assert "sum to" in _lib.last_error()


def test_plan_create_mesh_wide_mesh_needs_a_device_not_a_narrower_front():
    """Without a GPU a wide mesh now fails for want of a device (ENODEV), not for its width: the tree route took it."""
    import ctypes as C

    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    desc, keep = mesh_desc(W.jittered_unit_square(56, 56), "elasticity")
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.hommx_plan_create_mesh(C.byref(h), C.byref(desc)) != 0
    assert "no HIP device" in _lib.last_error() and not h.value
