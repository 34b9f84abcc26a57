"""Unstructured periodic micro meshes, host side (no GPU): periodic matching, the generators, the symbolic phase of the mesh route
(hommx_mesh_analyze) and its argument checks, create_mesh, and the test-side reference tests/periodic_fem.py pinned against the
oracle on structured meshes."""

import ctypes as C

import numpy as np
import pytest

import periodic_fem as PF
from hommx_amd import _lib, fem, mesh as Mm, workloads as W
from hommx_amd.batch import mesh_analyze, mesh_desc
from hommx_amd.cell_problem import create_periodic_boundary_conditions

GENERATORS = {
    "jittered_square": lambda: W.jittered_unit_square(12, 7, seed=1),
    "layered_square": lambda: W.layered_unit_square([0.3, 0.71], 10, 12, seed=2),
    "jittered_cube": lambda: W.jittered_unit_cube(3, 4, 3, seed=3),
    "square_nx_ne_ny": lambda: Mm.create_unit_square(9, 5),
}


def _constraint(msh):
    return create_periodic_boundary_conditions(fem.FunctionSpace(msh, 1))


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_periodic_matching(name):
    msh = GENERATORS[name]()
    d = msh.topology.dim
    c = _constraint(msh)
    x = msh.geometry.x[:, :d]
    on_max = np.isclose(x, 1.0).any(axis=1)
    assert c.num_independent == int((~on_max).sum())
    assert c.slaves.size == int(on_max.sum())
    # every slave lands on an independent node with the same folded coordinate
    assert not np.isclose(x[c.masters], 1.0).any()
    assert np.allclose(np.where(np.isclose(x[c.slaves], 1.0), 0.0, x[c.slaves]), x[c.masters])
    assert np.array_equal(np.sort(np.unique(c.to_periodic)), np.arange(c.num_independent))
    el = c.to_periodic[msh.cells]
    assert (np.sort(el, axis=1)[:, 1:] != np.sort(el, axis=1)[:, :-1]).all(), "an element repeats a periodic node"
    # the test-side matching agrees up to numbering
    node, nn = PF.periodic_map(msh.geometry.x, d)
    assert nn == c.num_independent
    assert len(set(zip(node.tolist(), c.to_periodic.tolist()))) == nn


@pytest.mark.parametrize("dim,n", [(2, 5), (3, 3)])
def test_structured_matching_unchanged(dim, n):
    msh = Mm.create_unit_square(n, n) if dim == 2 else Mm.create_unit_cube(n, n, n)
    from oracle import hommx_oracle as O

    c = _constraint(msh)
    assert np.array_equal(c.to_periodic, O.periodic_master_map(dim, n))
    s, m = O.periodic_slaves_masters(dim, n)
    assert np.array_equal(c.slaves, s) and np.array_equal(c.masters, m)


def test_non_periodic_mesh_raises():
    msh = W.jittered_unit_square(6, 6, seed=0)
    x = msh.geometry.x.copy()
    top = np.nonzero(np.isclose(x[:, 1], 1.0) & (x[:, 0] > 0.01) & (x[:, 0] < 0.99))[0]
    x[top[0], 0] += 0.02  # one top vertex without its bottom image
    bad = Mm.create_mesh(msh.cells, x[:, :2])
    with pytest.raises(ValueError, match=f"node {top[0]} "):
        _constraint(bad)


def test_generators_positive_volumes():
    for name, g in GENERATORS.items():
        msh = g()
        assert msh.shape == () or name == "square_nx_ne_ny"
        assert np.isclose(msh.cell_volumes().sum(), 1.0)
        X = msh.cell_vertices()
        if name != "square_nx_ne_ny":
            assert (np.linalg.det(X[:, 1:] - X[:, :1]) > 0).all()


def test_layered_mesh_conforms():
    msh = W.layered_unit_square([0.3, 0.71], 10, 12)
    yb = msh.cell_vertices()[:, :, 1]
    for s in (0.3, 0.71):
        assert not ((yb.min(axis=1) < s - 1e-12) & (yb.max(axis=1) > s + 1e-12)).any()


def test_create_mesh_validated():
    x = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], float)
    m = Mm.create_mesh(np.array([[0, 1, 3], [0, 3, 2]]), x)
    assert m.shape == () and m.topology.dim == 2 and m.geometry.x.shape == (4, 3)
    with pytest.raises(ValueError):
        Mm.create_mesh(np.array([[0, 1, 4]]), x)
    with pytest.raises(ValueError):
        Mm.create_mesh(np.array([[0, 1, 1]]), x)
    with pytest.raises(ValueError):
        Mm.create_mesh(np.array([[0, 1]]), x)
    with pytest.raises(ValueError):
        Mm.create_mesh(np.array([[0.0, 1.0, 2.0]]), x)
    with pytest.raises(ValueError):
        Mm.create_mesh(np.array([[0, 1, 2]]), np.full((4, 2), np.nan))
    with pytest.raises(ValueError, match="micro mesh must be"):
        Mm.micro_cells_per_side(m)


def _recount(msh, kind, order):
    """NumPy restatement of the symbolic phase: front width (unknowns) and sum over pivots of f^2 + 2 f t."""
    d = msh.topology.dim
    el = _constraint(msh).to_periodic[msh.cells]
    n = el.max() + 1
    bs = 1 if kind.startswith("poisson") else d
    t = d if kind.startswith("poisson") else d * (d + 1) // 2
    pos = np.empty(n, int)
    pos[order] = np.arange(n)
    first = pos[el].min(axis=1)
    birth = np.full(n, n)
    np.minimum.at(birth, el.ravel(), np.repeat(first, el.shape[1]))
    width, fl = 0, 0.0
    for k in range(n - 1):
        live = (birth <= k) & (pos >= k)
        live[order[-1]] = False
        a = int(live.sum())
        width = max(width, a * bs)
        for c in range(bs):
            f = a * bs - c
            fl += f * f + 2.0 * f * t
    return width, fl


@pytest.mark.parametrize("name,kind", [("jittered_square", "poisson"), ("layered_square", "elasticity"), ("jittered_cube", "poisson"),
                                       ("jittered_cube", "elasticity_voigt"), ("square_nx_ne_ny", "poisson_matrix")])
def test_analyze_matches_recount(name, kind, rng):
    msh = GENERATORS[name]()
    n = _constraint(msh).num_independent
    order = rng.permutation(n)
    w, fl = mesh_analyze(msh, kind, order=order)
    assert (w, fl) == _recount(msh, kind, order)
    # the library's own order is never wider than a random one, and its report is the recount of SOME permutation
    w0, _ = mesh_analyze(msh, kind)
    assert 0 < w0 <= w


def test_default_order_front_widths():
    """The widths the route's documentation and tools/bench_mesh.py quote (coordinate sweep: two cross-sections)."""
    assert mesh_analyze(W.jittered_unit_square(32, 32), "poisson")[0] <= 80
    assert mesh_analyze(W.jittered_unit_square(40, 40), "elasticity")[0] <= _lib.MESH_MAX_FRONT
    assert mesh_analyze(Mm.create_unit_cube(4, 4, 4), "elasticity")[0] <= _lib.MESH_MAX_FRONT


def _analyze_desc(desc):
    lib = _lib.load()
    w, fl = C.c_int32(0), C.c_double(0.0)
    rc = lib.hommx_mesh_analyze(C.byref(desc), C.byref(w), C.byref(fl))
    return rc, _lib.last_error(), w.value


def test_einval_bad_order():
    msh = W.jittered_unit_square(6, 6)
    n = _constraint(msh).num_independent
    order = np.arange(n)
    order[3] = 5
    with pytest.raises(_lib.HommxLibraryError, match="permutation"):
        mesh_analyze(msh, "poisson", order=order)


def test_einval_degenerate_element():
    msh = W.jittered_unit_square(6, 6)
    desc, keep = mesh_desc(msh, "poisson")
    keep["el_x"][4, 2] = 0.5 * (keep["el_x"][4, 0] + keep["el_x"][4, 1])  # flat triangle
    rc, msg, _ = _analyze_desc(desc)
    assert rc == -1 and "element 4 is degenerate" in msg


def test_einval_volume_not_one():
    msh = W.jittered_unit_square(6, 6)
    desc, keep = mesh_desc(msh, "poisson")
    keep["el_x"] *= 1.01
    rc, msg, _ = _analyze_desc(desc)
    assert rc == -1 and "sum to" in msg


def test_einval_node_range_and_repeats():
    msh = W.jittered_unit_square(6, 6)
    desc, keep = mesh_desc(msh, "poisson")
    keep["el_nodes"][0, 0] = desc.n_nodes
    rc, msg, _ = _analyze_desc(desc)
    assert rc == -1 and "out of range" in msg
    keep["el_nodes"][0, 0] = keep["el_nodes"][0, 1]
    rc, msg, _ = _analyze_desc(desc)
    assert rc == -1 and "appears twice" in msg


def test_einval_front_over_limit():
    msh = W.jittered_unit_square(56, 56)
    with pytest.raises(_lib.HommxLibraryError, match=rf"front width \d+ .* HOMMX_MESH_MAX_FRONT = {_lib.MESH_MAX_FRONT}"):
        mesh_analyze(msh, "elasticity")


def test_plan_create_mesh_validates_before_the_device():
    """hommx_plan_create_mesh rejects a bad mesh with EINVAL whether or not a GPU is present."""
    msh = W.jittered_unit_square(6, 6)
    desc, keep = mesh_desc(msh, "poisson")
    keep["el_x"] *= 1.01
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.hommx_plan_create_mesh(C.byref(h), C.byref(desc)) == -1
    assert "sum to" in _lib.last_error() and not h.value


def _coef(kind, dim, ne, rng):
    t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
    if kind == "poisson":
        return rng.uniform(0.5, 2.0, ne)
    if kind == "poisson_matrix":
        L = rng.normal(size=(ne, dim, dim)) * 0.3 + np.eye(dim)
        A = L @ L.transpose(0, 2, 1)
        return np.stack([A[:, k, l] for k, l in PF.PAIRS[dim]], 1)
    if kind == "elasticity":
        return np.stack([rng.uniform(0.5, 2.0, ne), rng.uniform(0.5, 2.0, ne)], 1)
    L = rng.normal(size=(ne, t, t)) * 0.3 + 2 * np.eye(t)
    V = L @ L.transpose(0, 2, 1)
    iu = np.triu_indices(t)
    return V[:, iu[0], iu[1]]


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 3)])
@pytest.mark.parametrize("kind", ["poisson", "poisson_matrix", "elasticity", "elasticity_voigt"])
@pytest.mark.parametrize("strat", [False, True])
def test_reference_helper_matches_oracle(dim, n, kind, strat, rng):
    from oracle import hommx_oracle as O

    msh = Mm.create_unit_square(n, n) if dim == 2 else Mm.create_unit_cube(n, n, n)
    coef = _coef(kind, dim, msh.num_cells, rng)
    M = np.eye(dim) + 0.2 * rng.normal(size=(dim, dim)) if strat else None
    AH, chi, node = PF.solve_cell(msh, kind, coef, M)
    okind = "poisson" if kind.startswith("poisson") else "elasticity"
    oc = coef if kind in ("poisson", "elasticity") else PF.material_tensor(kind, coef, dim)
    cp = O.build_cell_problem(okind, dim, n, oc, M)
    ref = O.effective_tensor(cp)
    assert np.abs(AH - ref).max() <= 1e-12 * np.abs(ref).max()
    # correctors: same functions up to constants, on the oracle's torus numbering
    chi_o = O.solve_correctors(cp)  # [n_dof, t]
    bs = cp.bs
    per_vertex = chi.reshape(chi.shape[0], -1, bs)[:, node]          # [t, n_vertices, bs]
    per_vertex_o = chi_o.T.reshape(chi.shape[0], -1, bs)[:, O.periodic_master_map(dim, n)]
    diff = per_vertex - per_vertex_o
    diff -= diff.mean(axis=1, keepdims=True)
    assert np.abs(diff).max() <= 1e-10 * max(1.0, np.abs(per_vertex_o).max())
