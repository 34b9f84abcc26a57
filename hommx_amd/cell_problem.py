"""Periodic cell problems on the unit square / cube -- the counterpart of ``hommx.cell_problem``
(/root/reference/src/hommx/cell_problem.py).

The reference builds the periodic identification with ``dolfinx_mpc`` (slave dofs on the max faces, masters on the
min faces; doubly / triply constrained edges and the corner handled separately so that no slave is a master:
cell_problem.py:38-136 in 2D, :139-300 in 3D) and re-creates a ``PeriodicLinearProblem`` (MPC assembly + null space +
KSP solve + back substitution, cell_problem.py:303-388) for every right-hand side of every macro cell.  On the structured
unit-cell mesh the net effect of the constraint is the torus map ``(i, j[, k]) -> (i mod n, j mod n[, k mod n])``; here it
is an index table built once per micro-mesh size, and the solve is one batched GPU call (``hommx_amd.batch``).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import fem
from .batch import MicroCellPlan
from .mesh import Mesh, micro_cells_per_side


@dataclass
class PeriodicConstraint:
    """What ``dolfinx_mpc.MultiPointConstraint`` holds after ``finalize()`` for the periodic unit cell.

    ``slaves`` / ``masters`` are node indices of the micro mesh (blocked: dof = node * bs + component);
    ``to_periodic[node]`` is the index of the independent unknown the node is identified with, ``num_independent`` = n^d.
    """

    function_space: fem.FunctionSpace
    slaves: np.ndarray
    masters: np.ndarray
    to_periodic: np.ndarray
    num_independent: int

    def backsubstitution(self, periodic_values: np.ndarray) -> np.ndarray:
        """Values at the independent unknowns -> values at all mesh nodes (``mpc.backsubstitution``, cell_problem.py:386)."""
        bs = self.function_space.bs
        v = np.asarray(periodic_values).reshape(self.num_independent, bs)
        return v[self.to_periodic].ravel()


def create_periodic_boundary_conditions(function_space: fem.FunctionSpace, bcs=None) -> PeriodicConstraint:
    """Periodic boundary condition on the unit square or unit cube (cell_problem.py:16-35).

    Every node on a max face is a slave of its image on the min faces: faces first (cell_problem.py:113-120, 237-245), then
    the doubly constrained edges (:248-295) and the (triply) constrained corner (:123-134, :276-298).  ``bcs`` is accepted
    for signature compatibility and ignored, as in the reference.
    """
    msh: Mesh = function_space.mesh
    d = msh.topology.dim
    if d == 1:
        raise ValueError("Periodic boundary conditions in 1d not implemented.")  # cell_problem.py:27-28
    if d not in (2, 3):
        raise ValueError(f"Unkown topology dimension. {d=} is something unexpected")
    try:
        n = micro_cells_per_side(msh)
    except ValueError:
        return _match_periodic(function_space)
    x = msh.geometry.x[:, :d]
    lo, hi = x.min(axis=0), x.max(axis=0)
    on_max = np.isclose(x, hi)
    slaves = np.nonzero(on_max.any(axis=1))[0]
    g = np.rint((x - lo) / (hi - lo) * n).astype(np.int64)
    gm = g[slaves].copy()
    gm[on_max[slaves]] = 0
    stride = (n + 1) ** np.arange(d)
    masters = gm @ stride
    to_periodic = (g % n) @ (n ** np.arange(d))
    return PeriodicConstraint(function_space, slaves, masters, to_periodic, n**d)


def _match_periodic(function_space: fem.FunctionSpace) -> PeriodicConstraint:
    """Any simplicial mesh of the unit cell: every node on a max face is matched geometrically with its image on the min faces, all
    coordinates on a max face folded at once (edges and corners land on the one independent node of their class).  The independent
    nodes are the nodes on no max face, numbered in mesh order."""
    from scipy.spatial import cKDTree

    msh: Mesh = function_space.mesh
    d = msh.topology.dim
    x = msh.geometry.x[:, :d]
    lo, hi = x.min(axis=0), x.max(axis=0)
    tol = 1e-8 * float((hi - lo).max())
    on_max = np.abs(x - hi) <= tol
    slaves = np.nonzero(on_max.any(axis=1))[0]
    indep = np.nonzero(~on_max.any(axis=1))[0]
    y = x[slaves].copy()
    y[on_max[slaves]] = np.broadcast_to(lo, y.shape)[on_max[slaves]]
    dist, j = cKDTree(x[indep]).query(y, distance_upper_bound=tol)
    miss = np.nonzero(~np.isfinite(dist))[0]
    if miss.size:
        s = int(slaves[miss[0]])
        raise ValueError(f"micro mesh is not periodic: node {s} at {x[s].tolist()} has no image on the min faces")
    masters = indep[j]
    to_periodic = np.empty(x.shape[0], dtype=np.int64)
    to_periodic[indep] = np.arange(indep.size)
    to_periodic[slaves] = j
    return PeriodicConstraint(function_space, slaves, masters, to_periodic, int(indep.size))


class PeriodicLinearProblem:
    """One periodic cell problem ``a(chi, z) = -l_m(z)`` for all canonical loads m at once -- the role of
    ``PeriodicLinearProblem`` (cell_problem.py:303-388) for the bilinear forms of ``hommx.hmm``.

    The reference takes UFL forms ``a`` and ``L``; without UFL the problem is described by its kind and data:

        kind   'poisson' | 'poisson_matrix' | 'elasticity' | 'elasticity_voigt'      (hmm.py:644-650 / 891-903)
        coef   element means of the coefficient on the micro mesh, in mesh element order
        M      optional Dtheta^T (stratified forms, hmm.py:759-772 / 1032-1048)
        loads  optional P[n_loads, n_el, t]: further linear forms l(z) = sum_K |K| P_K . eps(z)_K, a prescribed flux / stress per micro
               element (components in the order of ``Reconstruction.flux``, shear not doubled) -- the general ``L`` of the
               reference restricted to P1, where only element means of such a field matter.  An unstructured mesh then takes the
               tree route of the mesh family (a frontal plan has a load solve only with ``load_solve=True``; this class keeps the tree)

    ``solve()`` returns one ``fem.Function`` per canonical load on the micro mesh (slave nodes filled by back substitution,
    constants projected out as the reference's null-space handling does, cell_problem.py:349-361, 382) and stores the
    effective tensor in ``effective_tensor``.  With ``loads`` it also leaves their correctors ``a(chi_l, z) = -l_l(z)`` in
    ``load_correctors`` (one ``fem.Function`` per load) and the mean total flux of every load in ``effective_polarisation[n_loads, t]``.
    ``petsc_options`` is accepted and ignored (direct factorisation).
    """

    def __init__(self, kind: str, coef: np.ndarray, mpc: PeriodicConstraint, M: np.ndarray | None = None,
                 petsc_options: dict | None = None, device: int = 0, loads: np.ndarray | None = None):
        self._mpc = mpc
        self._kind = kind
        msh = mpc.function_space.mesh
        self._dim = msh.topology.dim
        self._coef = np.asarray(coef, dtype=float)[None]
        self._M = None if M is None else np.asarray(M, dtype=float)[None]
        try:
            self._n = micro_cells_per_side(msh)
        except ValueError:  # unstructured (or nx != ny) micro mesh: the mesh route, on the constraint's periodic numbering
            self._n = None
            self._plan = MicroCellPlan.from_mesh(msh, kind, device=device, constraint=mpc, route=None if loads is None else "tree")
        else:
            self._plan = MicroCellPlan(self._dim, self._n, kind, device=device)
        self.effective_tensor: np.ndarray | None = None
        self.info: int | None = None
        self._loads = None
        if loads is not None:
            self._loads = np.ascontiguousarray(loads, dtype=float)
            if self._loads.ndim != 3 or self._loads.shape[1:] != (self._plan.n_el, self._plan.t):
                raise ValueError(f"loads has shape {self._loads.shape}; expected (n_loads, {self._plan.n_el}, {self._plan.t})")
        self.load_correctors: list[fem.Function] | None = None
        self.effective_polarisation: np.ndarray | None = None

    def _functions(self, chi: np.ndarray) -> list[fem.Function]:
        """chi[k, n_periodic * bs] as functions on the micro mesh, slave nodes filled by back substitution."""
        out = []
        for m in range(chi.shape[0]):
            f = fem.Function(self._mpc.function_space)
            f.x.array[:] = self._mpc.backsubstitution(chi[m])
            out.append(f)
        return out

    def solve(self) -> list[fem.Function]:
        AH, chi, info = self._plan.solve(self._coef, self._M, return_info=True, return_correctors=True)
        self.effective_tensor, self.info = AH[0], int(info[0])
        if self._loads is not None:  # t loads per call
            t = self._plan.t
            parts = [self._plan.loads(self._coef, self._loads[b:b + t], self._M, return_correctors=True) for b in range(0, len(self._loads), t)]
            self.load_correctors = self._functions(np.concatenate([r.correctors[0] for r in parts]))
            self.effective_polarisation = np.concatenate([r.P_eff[0] for r in parts])
        return self._functions(chi[0])
