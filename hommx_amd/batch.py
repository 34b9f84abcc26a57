"""Batched micro-cell solves: the Python face of the C ABI.

``MicroCellPlan.solve`` replaces the macro-cell loop of ``BaseHMM._assemble_stiffness``
(/root/reference/src/hommx/hmm.py:298-332): one call returns the effective tensor of every
macro cell of the batch.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

KINDS = {
    "poisson": _lib.KIND_POISSON_SCALAR,
    "poisson_matrix": _lib.KIND_POISSON_MATRIX,
    "elasticity": _lib.KIND_ELASTICITY_ISO,
    "elasticity_voigt": _lib.KIND_ELASTICITY_VOIGT,
}


def mesh_desc(msh, kind: str, device: int = 0, order=None, constraint=None, flags: int = 0):
    """hommx_mesh_desc of a unit-cell mesh: periodic node of every element vertex + unfolded coordinates.  Returns (desc, arrays the
    descriptor points into -- keep them alive while it is used)."""
    from . import fem
    from .cell_problem import create_periodic_boundary_conditions

    if constraint is None:
        constraint = create_periodic_boundary_conditions(fem.FunctionSpace(msh, 1))
    d = msh.topology.dim
    to_periodic = np.asarray(constraint.to_periodic, dtype=np.int64)
    keep = {
        "to_periodic": to_periodic,
        "el_nodes": np.ascontiguousarray(to_periodic[msh.cells], dtype=np.int32),
        "el_x": np.ascontiguousarray(msh.geometry.x[msh.cells][:, :, :d], dtype=np.float64),
    }
    if order is not None:
        keep["order"] = np.ascontiguousarray(order, dtype=np.int32)
    desc = _lib.MeshDesc(d, KINDS[kind], int(device), int(flags), int(constraint.num_independent), int(msh.cells.shape[0]),
                         keep["el_nodes"].ctypes.data, keep["el_x"].ctypes.data,
                         keep["order"].ctypes.data if order is not None else None)
    return desc, keep


def mesh_analyze(msh, kind: str = "poisson", order=None, constraint=None) -> tuple[int, float]:
    """(front width in unknowns, flops per solve) of the mesh route for this mesh and order -- host only, no GPU
    (hommx_mesh_analyze).  Raises HommxLibraryError (code -1, HOMMX_EINVAL) with the reason for a mesh the route cannot take."""
    desc, keep = mesh_desc(msh, kind, 0, order, constraint)
    lib = _lib.load()
    w, fl = C.c_int32(0), C.c_double(0.0)
    _lib.check(lib.hommx_mesh_analyze(C.byref(desc), C.byref(w), C.byref(fl)), "hommx_mesh_analyze")
    return int(w.value), float(fl.value)


def mesh_analyze_tree(msh, kind: str = "poisson", constraint=None) -> dict:
    """The tree route's symbolic phase for this mesh (hommx_mesh_analyze_tree) -- host only, no GPU.  Returns n_fronts, n_groups,
    max_front (largest front, unknowns), flops_per_solve (multifrontal model), supernode_of_node[n_nodes] and parent[n_fronts] (supernodes
    in elimination order, children first, parent -1 at the root).  Raises HommxLibraryError (HOMMX_EINVAL) for a mesh it cannot take."""
    desc, keep = mesh_desc(msh, kind, 0, None, constraint)
    lib = _lib.load()
    nf, ng, mx, fl = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    sn = np.empty(int(desc.n_nodes), dtype=np.int32)
    _lib.check(lib.hommx_mesh_analyze_tree(C.byref(desc), C.byref(nf), C.byref(ng), C.byref(mx), C.byref(fl), sn.ctypes.data, None),
               "hommx_mesh_analyze_tree")
    parent = np.empty(int(nf.value), dtype=np.int32)
    _lib.check(lib.hommx_mesh_analyze_tree(C.byref(desc), None, None, None, None, None, parent.ctypes.data), "hommx_mesh_analyze_tree")
    return {"n_fronts": int(nf.value), "n_groups": int(ng.value), "max_front": int(mx.value), "flops_per_solve": float(fl.value),
            "supernode_of_node": sn, "parent": parent}


@dataclass
class Reconstruction:
    """Micro fields of macro cells reconstructed from their correctors (include/hommx_hip.h, hommx_reconstruct_batch).

    ``xi[N, t]``: the macro gradient / engineering-Voigt strain of every cell.  ``mean_strain`` / ``mean_flux`` ``[N, t]``: sum |K| s_K and
    sum |K| q_K over the micro elements; ``energy[N]``: sum |K| s_K . q_K; ``max_flux[N]``: the largest |q_K| (Frobenius norm of the stress
    for elasticity) and ``argmax_element[N]`` the smallest element reaching it.  ``strain`` / ``flux`` ``[N, n_el, t]`` or None.  On the
    discrete problem mean_strain = xi, mean_flux = A_eff xi and energy = xi . A_eff xi.  ``cells``: the macro cells (``BaseHMM.reconstruct``).

    With regions (hommx_reconstruct_source; R of them): ``region_volume[N, R]`` the volume of the elements labelled r, ``region_mean_strain`` /
    ``region_mean_flux`` ``[N, R, t]`` their sums divided by that volume (NaN where it is 0), ``region_energy[N, R]`` the region's part of
    ``energy`` (not divided: the regions of a cover sum to it), ``region_max_flux[N, R]`` the largest |q_K| in the region (-1 in an empty one)
    and ``region_argmax_element[N, R]`` the smallest of its elements reaching it (-1)."""

    xi: np.ndarray
    mean_strain: np.ndarray
    mean_flux: np.ndarray
    energy: np.ndarray
    max_flux: np.ndarray
    argmax_element: np.ndarray
    A_eff: np.ndarray
    info: np.ndarray
    strain: np.ndarray | None = None
    flux: np.ndarray | None = None
    cells: np.ndarray | None = None
    region_volume: np.ndarray | None = None
    region_mean_strain: np.ndarray | None = None
    region_mean_flux: np.ndarray | None = None
    region_energy: np.ndarray | None = None
    region_max_flux: np.ndarray | None = None
    region_argmax_element: np.ndarray | None = None
    secant = None  # an attribute, not a field: reconstruct(nonlinear=True) of the solver classes sets the SecantResult of its micro iteration

    @classmethod
    def from_stats(cls, xi, stats, A_eff, info, strain=None, flux=None, cells=None, region_stats=None) -> "Reconstruction":
        """From the library's rows: stats[N, 2t + 3] and, with regions, region_stats[N, R, 2t + 4] = [volume | sums | max | argmax], whose
        sums are not divided by the volume."""
        t = xi.shape[1]
        r = cls(xi, stats[:, :t].copy(), stats[:, t:2 * t].copy(), stats[:, 2 * t].copy(), stats[:, 2 * t + 1].copy(),
                stats[:, 2 * t + 2].astype(np.int64), A_eff, info, strain, flux, cells)
        if region_stats is not None:
            vol = region_stats[:, :, 0].copy()
            inv = np.full_like(vol, np.nan)
            np.divide(1.0, vol, out=inv, where=vol > 0)
            r.region_volume = vol
            r.region_mean_strain = region_stats[:, :, 1:1 + t] * inv[:, :, None]
            r.region_mean_flux = region_stats[:, :, 1 + t:1 + 2 * t] * inv[:, :, None]
            r.region_energy = region_stats[:, :, 1 + 2 * t].copy()
            r.region_max_flux = region_stats[:, :, 2 + 2 * t].copy()
            r.region_argmax_element = region_stats[:, :, 3 + 2 * t].astype(np.int64)
        return r


@dataclass
class Sensitivities:
    """Derivatives of A_H of macro cells with respect to the micro coefficient (include/hommx_hip.h, hommx_sensitivity_source).

    ``dA[N, n_dirs, t, t]``: the derivative of A_H along every direction (a perturbation of the element stream), symmetric in its last two
    axes; ``grad[N, n_el(, n_comp)]`` or None: the per-element gradient of ``weights : A_H``, shaped like the coefficient, with
    sum grad * dir = weights : dA[dir]; ``A_eff[N, t, t]`` and ``info[N]`` as ``solve`` returns them.  ``names`` / ``cells``: what the
    directions are called and the macro cells (``BaseHMM.tensor_derivatives``)."""

    dA: np.ndarray
    grad: np.ndarray | None
    A_eff: np.ndarray
    info: np.ndarray
    names: tuple | None = None
    cells: np.ndarray | None = None


@dataclass
class SecondSensitivities:
    """Second derivatives of A_H of macro cells along coefficient directions (include/hommx_hip.h, hommx_second_sensitivity_source;
    DESIGN 4.13).

    ``d2A[N, n_dirs, n_dirs, t, t]``: d^2 A_H / d theta_a d theta_b for the perturbation coef + theta_a dir_a + theta_b dir_b of the element
    stream, exact on the discrete problem, symmetric bitwise in its last two axes and in (a, b); every ``d2A[:, a, a]`` is negative
    semidefinite.  ``dA[N, n_dirs, t, t]`` or None: the first derivatives along the same directions, the bits ``sensitivities`` returns;
    ``A_eff[N, t, t]`` and ``info[N]`` as ``solve`` returns them.  ``names`` / ``cells``: what the directions are called and the macro
    cells (``BaseHMM.tensor_second_derivatives``)."""

    d2A: np.ndarray
    dA: np.ndarray | None
    A_eff: np.ndarray
    info: np.ndarray
    names: tuple | None = None
    cells: np.ndarray | None = None


@dataclass
class StratSensitivities:
    """Derivatives of A_H of macro cells with respect to the stratification M = Dtheta^T (include/hommx_hip.h,
    hommx_stratification_sensitivity_source).

    ``dA_dM[N, d, d, t, t]`` or None: the derivative of A_H[m, n] with respect to M[a, b], symmetric in its last two axes;
    ``grad_M[N, d, d]`` or None: sum_mn weights[m, n] dA_dM[a, b, m, n], the gradient of ``weights : A_H`` with respect to M;
    ``A_eff[N, t, t]`` and ``info[N]`` as ``solve`` returns them.  ``cells``: the macro cells; with design parameters
    (``BaseHMM.stratification_derivatives``) ``names`` and ``dA[N, n_params, t, t]``, the derivative of A_H along each."""

    dA_dM: np.ndarray | None
    grad_M: np.ndarray | None
    A_eff: np.ndarray
    info: np.ndarray
    cells: np.ndarray | None = None
    names: tuple | None = None
    dA: np.ndarray | None = None


@dataclass
class LoadResponse:
    """Effective polarisation and response of macro cells to user-supplied loads P (include/hommx_hip.h, hommx_loads_source).

    ``P_eff[N, n_loads, t]``: the mean total flux / stress of every load, by Levin's identity from the canonical correctors (every plan);
    ``A_eff[N, t, t]`` and ``info[N]`` of that canonical pass.  With ``response`` (a solve for the loads themselves): ``energy[N, n_loads,
    n_loads]`` = sum |K| eps(chi_l) . material eps(chi_l'), ``mean_flux[N, n_loads, t]`` (the mean of q = P + material eps(chi_l), equal
    to ``P_eff`` up to rounding), ``max_flux[N, n_loads]`` and ``argmax_element[N, n_loads]`` as ``Reconstruction`` defines them; with
    ``fields`` ``strain`` and ``flux`` ``[N, n_loads, n_el, t]``; with ``return_correctors`` ``correctors[N, n_loads, n_nodes * bs]``,
    mean-free.  ``cells``: the macro cells (``BaseHMM.load_response``).  What was not asked for is None."""

    P_eff: np.ndarray
    A_eff: np.ndarray
    info: np.ndarray
    energy: np.ndarray | None = None
    mean_flux: np.ndarray | None = None
    max_flux: np.ndarray | None = None
    argmax_element: np.ndarray | None = None
    strain: np.ndarray | None = None
    flux: np.ndarray | None = None
    correctors: np.ndarray | None = None
    cells: np.ndarray | None = None


@dataclass
class CriterionResult:
    """A failure criterion on the reconstructed micro state of macro cells (include/hommx_hip.h, hommx_criterion_source).

    ``max[N]``: the largest value v_K of the criterion over the micro elements and ``argmax_element[N]`` the smallest element reaching
    it (a NaN value never wins; -inf and -1 when every value is NaN); ``mean[N]``: sum |K| v_K over the unit cell (NaN when a value
    is); ``exceed_volume[N]``: the volume fraction of the elements with v_K >= threshold.  With ``values`` ``values[N, n_el]``, with
    ``fields`` ``strain`` and ``flux`` ``[N, n_el, t]``, the total state the criterion saw (a load included).  ``A_eff[N, t, t]`` and
    ``info[N]`` of the canonical pass.  ``cells``: the macro cells (``BaseHMM.criterion``).  What was not asked for is None."""

    max: np.ndarray
    argmax_element: np.ndarray
    mean: np.ndarray
    exceed_volume: np.ndarray
    A_eff: np.ndarray
    info: np.ndarray
    values: np.ndarray | None = None
    strain: np.ndarray | None = None
    flux: np.ndarray | None = None
    cells: np.ndarray | None = None
    secant = None  # an attribute, not a field: criterion(nonlinear=True) of the solver classes sets the SecantResult of its micro iteration


@dataclass
class SecantResult:
    """The secant iteration of a strain-dependent coefficient on macro cells (include/hommx_hip.h, hommx_secant_source),
    every member that of the cell's STOPPING round: ``A_eff[N, t, t]`` the secant tensor, ``mean_flux[N, t]`` = sum |K| q_K (= A_eff xi
    up to rounding), ``rounds[N]`` (int), ``change[N]`` = max |w - c| / max |w| of that round, ``status[N]`` (int: 0 converged,
    1 ``max_iter`` reached, 2 the law gave a value that is not finite, 3 the elimination flagged a pivot -- ``info`` then), ``info[N]``.
    With ``return_coef`` ``coef[N, n_el(, n_comp)]``, the element stream ``A_eff`` belongs to (pass it to ``reconstruct`` /
    ``criterion`` for the nonlinear state); with ``fields`` ``strain`` and ``flux`` ``[N, n_el, t]``; with ``values``
    ``values[N, n_el, n_comp]``, what the law gave.  ``cells``: the macro cells (solver classes).  What was not asked for is None.

    From ``secant_tangent`` (hommx_secant_tangent_source) also ``tangent[N, t, t]`` = D = d mean_flux / d xi at that
    state (NaN for a cell of status 2 or 3), ``asymmetry[N]`` = max |T - T^T| / max |T| of the element tangents (0 for a law with a
    potential; D is then exact, otherwise it is the tangent of the symmetrised law; NaN for status 2 or 3), ``tangent_info[N]`` the
    info of the tangent elimination and, with ``return_tangent_coef``, ``tangent_coef[N, n_el, t (t + 1) / 2]``, the element stream
    of the tangent kind that was eliminated.

    For a law with history variables ``history[N, n_el, n_history]``: the updates of the stopping round -- the input's
    bits for a cell of status 2 or 3 --, what the next load step takes as its ``history`` once the caller commits it.

    With ``secant(criterion=...)`` / ``secant(reconstruct=True)`` (hommx_secant_state_source) ``criterion``, a
    ``CriterionResult``, and ``reconstruction``, a ``Reconstruction``, of the state the iteration stopped in (their ``A_eff`` and
    ``info`` are this result's); what a cell of status 3 holds there means nothing."""

    A_eff: np.ndarray
    mean_flux: np.ndarray
    rounds: np.ndarray
    change: np.ndarray
    status: np.ndarray
    info: np.ndarray
    coef: np.ndarray | None = None
    strain: np.ndarray | None = None
    flux: np.ndarray | None = None
    values: np.ndarray | None = None
    cells: np.ndarray | None = None
    tangent: np.ndarray | None = None
    asymmetry: np.ndarray | None = None
    tangent_info: np.ndarray | None = None
    tangent_coef: np.ndarray | None = None
    history: np.ndarray | None = None
    criterion: CriterionResult | None = None
    reconstruction: Reconstruction | None = None


# The host entries of the nonlinear family (include/hommx_hip.h), by (tangent, the last part of history < load < state that is there),
# and what an entry of that part takes behind its argument struct: the parts before the last are optional there (None: NULL).  The
# device form of an entry has the suffix and takes the stream last.  There is no tangent entry with a state tail.
_SECANT_ENTRIES = {
    (False, None): "hommx_secant_source",
    (False, "history"): "hommx_secant_history_source",
    (False, "load"): "hommx_secant_load_source",
    (False, "state"): "hommx_secant_state_source",
    (True, None): "hommx_secant_tangent_source",
    (True, "history"): "hommx_secant_tangent_history_source",
    (True, "load"): "hommx_secant_tangent_load_source",
}
_SECANT_TAKES = {None: (), "history": ("history",), "load": ("history", "load"), "state": ("history", "load", "state")}


def _secant_entry(tangent: bool, hargs, largs, sargs, device: bool) -> tuple[str, tuple]:
    """The entry a call of the nonlinear family goes to -> (its name, its arguments behind the argument struct): ``hargs`` / ``largs`` /
    ``sargs`` the ``HistoryArgs`` / ``SecantLoadArgs`` / ``SecantStateArgs`` of the call, None for a part it does not have."""
    parts = {"history": hargs, "load": largs, "state": sargs}
    last = next((k for k in ("state", "load", "history") if parts[k] is not None), None)
    name = _SECANT_ENTRIES[bool(tangent), last] + ("_device" if device else "")
    return name, tuple(None if parts[k] is None else C.byref(parts[k]) for k in _SECANT_TAKES[last])


REGION_FIELDS = ("region_volume", "region_mean_strain", "region_mean_flux", "region_energy", "region_max_flux", "region_argmax_element")


def region_labels(labels, n_el: int, n_regions: int | None = None) -> tuple[np.ndarray, int]:
    """labels[n_el] (integers or bool) as the uint8 array the library takes, and the number of regions.  A label below 0 or above 254
    becomes 255; every label >= n_regions belongs to no region.  ``n_regions`` defaults to the largest label below
    HOMMX_RECON_MAX_REGIONS plus one."""
    lab = np.asarray(labels)
    if lab.dtype == bool:
        lab = lab.astype(np.uint8)
    if not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"region labels must be integers; got {lab.dtype}")
    if lab.shape != (n_el,):
        raise ValueError(f"regions has shape {lab.shape}; expected ({n_el},)")
    out = np.ascontiguousarray(np.where((lab >= 0) & (lab < 255), lab, 255).astype(np.uint8))
    if n_regions is None:
        used = out[out < _lib.RECON_MAX_REGIONS]
        if used.size == 0:
            raise ValueError(f"no region label below {_lib.RECON_MAX_REGIONS}")
        n_regions = int(used.max()) + 1
    if not 1 <= int(n_regions) <= _lib.RECON_MAX_REGIONS:
        raise ValueError(f"n_regions must be 1 .. {_lib.RECON_MAX_REGIONS}; got {n_regions}")
    return out, int(n_regions)


def _per_cell_code(per_cell, curvature: bool = False, argument: str = "per_cell") -> int:
    """per_cell of hommx_sens_args / hommx_sens2_args: 0 shared, 1 per cell, ``"parameters"`` HOMMX_DIRS_PARAMETERS or, with ``curvature``,
    HOMMX_DIRS_PARAMETERS_CURVATURE.  ``argument``: what the caller's method calls the argument that says ``"parameters"``."""
    code = _lib.DIRS_PARAMETERS if isinstance(per_cell, str) and per_cell == "parameters" else int(bool(per_cell))
    if curvature:
        if code != _lib.DIRS_PARAMETERS:
            raise ValueError(f'curvature=True needs {argument}="parameters": the curvature term is that of the program\'s own parameters')
        code = _lib.DIRS_PARAMETERS_CURVATURE
    return code


@dataclass(frozen=True)
class Program:
    """The postfix program of an expression coefficient (include/hommx_hip.h, hommx_coef_program; ``hommx_amd.expr.Expression.program``):
    ops[n_ops, 2] uint8 = (opcode, operand), consts[n_consts] float64, the number of components it stores, and how many of its first
    constants are parameters (``Expression(..., p=[...])``).  ``n_fields``: how many per-cell fields it reads
    (``Expression(..., fields=...)``; ``X k``, k >= 3) -- no member of hommx_coef_program: it travels in the source
    (hommx_coef_source.n_fields), with the rows [N_c, 3 + n_fields] it describes."""

    ops: np.ndarray
    consts: np.ndarray
    n_comp: int
    n_params: int = 0
    n_fields: int = 0

    def struct(self) -> "_lib.CoefProgram":
        """The hommx_coef_program that points into this program's arrays (host memory; keep ``self`` alive while it is in use)."""
        return _lib.CoefProgram(int(self.ops.shape[0]), int(self.consts.size), int(self.n_comp), int(self.n_params), self.ops.ctypes.data,
                                self.consts.ctypes.data if self.consts.size else None)


@dataclass(frozen=True)
class CoefStream:
    """The coefficient of a block of macro cells in one of the four forms the library takes (include/hommx_hip.h): sampled element means,
    phase mask + two values per cell, table of g + (a, b) per cell, program of an expression + quadrature points + midpoint per cell.  ``method`` names the plan's host method (``method + "_device"`` is its
    device twin), ``shared`` holds the arguments every cell shares in the order that method takes them, ``per_cell`` is the one array whose
    first axis is the macro cell: ``plan.<method>(*shared, per_cell, M, return_info=...)``."""

    method: str
    shared: tuple
    per_cell: np.ndarray

    @classmethod
    def sampled(cls, coef) -> "CoefStream":
        return cls("solve", (), np.ascontiguousarray(coef, dtype=np.float64))

    @classmethod
    def two_phase(cls, mask, values) -> "CoefStream":
        return cls("solve_two_phase", (np.ascontiguousarray(np.asarray(mask).astype(np.uint8)),), np.ascontiguousarray(values, dtype=np.float64))

    @classmethod
    def separable(cls, family: str, table, weights, params) -> "CoefStream":
        return cls("solve_separable", (family, np.ascontiguousarray(table, dtype=np.float64),
                                       None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)),
                   np.ascontiguousarray(params, dtype=np.float64))

    @classmethod
    def program(cls, points, weights, ops, consts, n_comp: int, midpoints, *, n_params: int = 0, n_fields: int = 0) -> "CoefStream":
        """An expression coefficient: points[n_el, n_q, dim] and weights[n_q] of the micro quadrature rule, the program of
        ``Expression.program()`` with its number of components, midpoints[N_c, 3 + n_fields] of the macro cells -- the midpoint, then
        the ``n_fields`` fields of the cell; ``n_params``: how many of the first constants are the expression's parameters."""
        prog = Program(np.ascontiguousarray(ops, dtype=np.uint8).reshape(-1, 2), np.ascontiguousarray(consts, dtype=np.float64).ravel(), int(n_comp),
                       int(n_params), int(n_fields))
        return cls("solve_program", (np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(weights, dtype=np.float64), prog),
                   np.ascontiguousarray(midpoints, dtype=np.float64))

    def __len__(self) -> int:
        return self.per_cell.shape[0]

    def coef_source(self, address=lambda a: a.ctypes.data) -> "_lib.CoefSource":
        """The stream as the hommx_coef_source of the entry points that take one: the one place that spells the four forms for them.
        ``address(array) -> pointer``: the array's own address (host entry; the stream keeps the arrays alive), or an upload.  The
        program of an expression is host memory either way; the source keeps its struct alive."""
        src = _lib.CoefSource()
        if self.method == "solve":
            src.form, src.coef = _lib.COEF_SAMPLED, address(self.per_cell)
        elif self.method == "solve_two_phase":
            src.form, src.mask, src.values = _lib.COEF_TWO_PHASE, address(self.shared[0]), address(self.per_cell)
        elif self.method == "solve_program":
            points, weights, prog = self.shared
            src.form, src.n_q, src.n_fields = _lib.COEF_PROGRAM, int(points.shape[1]), int(prog.n_fields)
            src.table, src.weights, src.params = address(points), address(weights), address(self.per_cell)
            src._program = (prog, prog.struct())  # ctypes keeps no reference to what a pointer member points at
            src.program = C.pointer(src._program[1])
        else:
            family, table, weights = self.shared
            src.form, src.table, src.params = _lib.COEF_SEPARABLE, address(table), address(self.per_cell)
            src.family = {"affine": _lib.SAMPLER_AFFINE, "reciprocal": _lib.SAMPLER_RECIPROCAL}[family]
            src.n_q = 1 if family == "affine" else int(table.shape[1])
            src.weights = None if weights is None or family == "affine" else address(weights)
        return src

    def block(self, b: int, e: int) -> "CoefStream":
        """Cells [b, e) of the stream (the shared arguments are shared, not copied)."""
        return CoefStream(self.method, self.shared, self.per_cell[b:e])

    def solve(self, plan, M, **kw):
        """Through the host method of ``plan`` (a MicroCellPlan or a stand-in that offers ``method``)."""
        return getattr(plan, self.method)(*self.shared, self.per_cell, M, **kw)

    def solve_device(self, plan: "MicroCellPlan", upload, M_ptr, out_ptr, info_ptr, stream):
        """Through ``plan.solve_source_device``: ``upload(array) -> device pointer`` copies every array of the stream that the library reads
        to the plan's device (``coef_source``)."""
        plan.solve_source_device(len(self), self.coef_source(upload), M_ptr, out_ptr, info_ptr, stream)


class MicroCellPlan:
    """Everything batch-independent for one (dim, n_micro, kind): kernel choice + device scratch.

    Replaces the per-right-hand-side ``dolfinx_mpc.LinearProblem`` construction of hmm.py:420-425.
    """

    load_sources = True  # loads() takes a program CoefStream as P and eigenstrain=True (what the solver classes ask a plan before they send either)

    def __init__(self, dim: int, n_micro: int, kind: str = "poisson", device: int = 0, flags: int = 0, tree_loads: bool = False):
        """``tree_loads``: a plan of the nested-dissection route ("multifrontal") does the load solves of ``loads(response=True)``,
        ``criterion``, ``secant`` with a load and ``second_sensitivities`` by substitution on the fronts its canonical pass has just left
        (HOMMX_FLAG_TREE_LOADS; ``load_kernel`` is then "multifrontal_subst") instead of a second elimination.  Off by default; without
        effect on every other route."""
        if kind not in KINDS:
            raise ValueError(f"unknown kind {kind!r}; expected one of {sorted(KINDS)}")
        self._lib = _lib.load()
        desc = _lib.PlanDesc(int(dim), int(n_micro), KINDS[kind], int(device), int(flags) | (_lib.FLAG_TREE_LOADS if tree_loads else 0))
        h = C.c_void_p()
        _lib.check(self._lib.hommx_plan_create(C.byref(h), C.byref(desc)), "hommx_plan_create")
        self._adopt(h, int(dim), int(n_micro), kind, device, int(n_micro) ** int(dim), None)

    @classmethod
    def from_mesh(cls, msh, kind: str = "poisson", device: int = 0, order=None, constraint=None, route: str | None = None,
                  load_solve: bool = False, tree_loads: bool = False) -> "MicroCellPlan":
        """Plan of the mesh route for ANY periodic simplicial mesh of the unit cell (include/hommx_hip.h, hommx_plan_create_mesh).

        The periodic nodes are those of ``create_periodic_boundary_conditions`` (or of ``constraint``, when given); ``to_periodic``
        maps every mesh vertex to its periodic node, and correctors are indexed by periodic node.  ``order``: elimination order of
        the periodic nodes (default: the library's reverse Cuthill-McKee).  coef[cell][el] follows the mesh's cell order.
        ``n_micro`` is None, ``front_width`` the width of the frontal elimination in unknowns (0 on the tree route).

        ``route``: None lets the library choose (the frontal route "mesh_front" up to a front of 192 unknowns, the nested-dissection route
        "mesh_multifrontal" beyond); "front" insists on the frontal route (HOMMX_EINVAL for a mesh too wide for it); "tree" takes the
        nested-dissection route for any mesh (``order`` is then ignored).

        ``load_solve``: a plan of the frontal route gets a load solve (HOMMX_MESH_FLAG_LOADS; ``load_kernel`` is then
        "mesh_front_subst": substitution on the pivot columns of its corrector arena) and with it the response outputs of ``loads`` and
        ``second_sensitivities``; without it such a plan refuses them.  Meaningless on the tree route, which has a load solve of its own:
        the flag is ignored there.  ``solve`` and the correctors do not depend on it.

        ``tree_loads``: a plan of the tree route does its load solves by substitution on the fronts its canonical pass has just left
        (HOMMX_MESH_FLAG_TREE_LOADS; ``load_kernel`` is then "mesh_multifrontal_subst") instead of a second elimination.  Off by
        default; without effect on the frontal route."""
        if kind not in KINDS:
            raise ValueError(f"unknown kind {kind!r}; expected one of {sorted(KINDS)}")
        if route not in (None, "front", "tree"):
            raise ValueError(f"unknown route {route!r}; expected None, 'front' or 'tree'")
        flags = ((_lib.MESH_FLAG_TREE if route == "tree" else 0) | (_lib.MESH_FLAG_LOADS if load_solve else 0)
                 | (_lib.FLAG_TREE_LOADS if tree_loads else 0))
        desc, keep = mesh_desc(msh, kind, device, order, constraint, flags=flags)
        self = cls.__new__(cls)
        self._lib = _lib.load()
        if route == "front":  # the frontal route's own analysis: its error (front too wide) instead of the tree route
            _lib.check(self._lib.hommx_mesh_analyze(C.byref(desc), None, None), "hommx_mesh_analyze")
        h = C.c_void_p()
        _lib.check(self._lib.hommx_plan_create_mesh(C.byref(h), C.byref(desc)), "hommx_plan_create_mesh")
        self._adopt(h, int(desc.dim), None, kind, device, int(desc.n_nodes), keep["to_periodic"])
        return self

    def _adopt(self, h, dim: int, n_micro: int | None, kind: str, device: int, n_nodes: int, to_periodic):
        """Take the handle of a created plan and read what the library decided for it."""
        self._h = h
        self.dim, self.n_micro, self.kind, self.device = dim, n_micro, kind, int(device)
        self.n_el = int(self._lib.hommx_plan_num_elements(h))
        self.n_comp = int(self._lib.hommx_plan_coef_components(h))
        self.t = int(self._lib.hommx_plan_tensor_size(h))
        self.kernel = self._lib.hommx_plan_kernel_name(h).decode()
        self.corrector_kernel = self._lib.hommx_plan_corrector_kernel_name(h).decode()  # the route of its corrector / reconstruct calls
        self.load_kernel = self._lib.hommx_plan_load_kernel_name(h).decode()  # the route of the load solve of loads(..., response=True)
        self.route_detail = self._lib.hommx_plan_route_detail(h).decode()  # what that route launches for this plan (reports)
        self.flops_per_solve = float(self._lib.hommx_plan_flops_per_solve(h))  # dense flops of the route, by its own model
        self.n_nodes = n_nodes  # periodic nodes (correctors: dof = node * bs + component)
        self.front_width = int(self._lib.hommx_plan_front_width(h))  # 0 unless the frontal mesh route
        self.to_periodic = to_periodic

    def reserve(self, n_cells: int):
        """Allocate the device workspace for batches of up to ``n_cells`` now (otherwise the first solve does it)."""
        _lib.check(self._lib.hommx_plan_reserve(self._h, int(n_cells)), "hommx_plan_reserve")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hommx_plan_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- host arrays -----------------------------------------------------------------------------
    @property
    def _el(self) -> tuple:
        """Shape of one cell's element stream: (n_el,) or (n_el, n_comp)."""
        return (self.n_el,) + ((self.n_comp,) if self.n_comp > 1 else ())

    @property
    def _bs(self) -> int:
        """Unknowns per periodic node."""
        return 1 if self.kind.startswith("poisson") else self.dim

    @staticmethod
    def _as_stream(coef) -> CoefStream:
        """``coef`` as every method below takes it -- an array of element means or a ``CoefStream`` -- as a stream."""
        return coef if isinstance(coef, CoefStream) else CoefStream.sampled(coef)

    def _check_coef(self, coef) -> tuple[np.ndarray, int]:
        """coef[N_c, n_el(, n_comp)] as contiguous float64, and N_c."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        nc = coef.shape[0]
        if coef.size != nc * self.n_el * self.n_comp:
            raise ValueError(f"coef has shape {coef.shape}; expected ({nc}, {self.n_el}" + (f", {self.n_comp})" if self.n_comp > 1 else ")"))
        return coef, nc

    def _check_M(self, M, nc: int) -> tuple[np.ndarray | None, int | None]:
        """M[N_c, d, d] as contiguous float64 and its address (the caller holds the array while the address is in use); None, None without M."""
        if M is None:
            return None, None
        M = np.ascontiguousarray(M, dtype=np.float64)
        if M.shape != (nc, self.dim, self.dim):
            raise ValueError(f"M has shape {M.shape}; expected ({nc}, {self.dim}, {self.dim})")
        return M, M.ctypes.data

    def _host_call(self, what: str, nc: int, M, call, return_info: bool = True):
        """Check ``M``, allocate A_eff[N_c, t, t] and info[N_c], run ``call(M address, A_eff address, info address) -> status`` of the host
        entry point ``what`` unless the batch is empty; returns (A_eff, info), or A_eff alone."""
        M, Mp = self._check_M(M, nc)
        out = np.empty((nc, self.t, self.t), dtype=np.float64)
        info = np.zeros(nc, dtype=np.int32)
        if nc:
            _lib.check(call(Mp, out.ctypes.data, info.ctypes.data), what)
        return (out, info) if return_info else out

    def _source_call(self, what: str, nc: int, M, stream: "CoefStream", args):
        """``_host_call`` of a host entry point that takes (plan, N_c, source, M, argument struct): A_eff and info go into ``args``."""
        src = stream.coef_source()

        def call(Mp, o, i):
            args.A_eff, args.info = o, i
            return getattr(self._lib, what)(self._h, nc, C.byref(src), Mp, C.byref(args))

        return self._host_call(what, nc, M, call)

    def _check_directions(self, directions, nc: int, per_cell: bool) -> tuple[np.ndarray, int]:
        """directions[(N_c,) n_dirs, n_el(, n_comp)] as float64 -> (directions, n_dirs)."""
        el = self._el
        dirs = np.ascontiguousarray(directions, dtype=np.float64)
        lead = ((nc,) if per_cell else ())
        nd = dirs.shape[len(lead)] if dirs.ndim == len(lead) + 1 + len(el) else -1
        if nd < 0 or dirs.shape != lead + (nd,) + el:
            raise ValueError(f"directions has shape {dirs.shape}; expected {lead + ('n_dirs',) + el}")
        if not 1 <= nd <= _lib.SENS_MAX_DIRS:
            raise ValueError(f"n_dirs must be 1 .. {_lib.SENS_MAX_DIRS}; got {nd}")
        return dirs, nd

    @staticmethod
    def _parameter_count(coef) -> int:
        """The differentiable slots of ``directions="parameters"``, n_params + n_fields: the coefficient must be a program ``CoefStream``
        with parameters or fields."""
        prog = coef.shared[2] if isinstance(coef, CoefStream) and coef.method == "solve_program" else None
        if prog is None or prog.n_params + prog.n_fields < 1:
            raise ValueError('directions="parameters" needs the CoefStream of an expression with parameters (CoefStream.program(..., n_params=...))')
        return int(prog.n_params + prog.n_fields)

    def _check_weights(self, weights, nc: int) -> np.ndarray:
        """weights[N_c, t, t] as float64."""
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (nc, self.t, self.t):
            raise ValueError(f"weights has shape {weights.shape}; expected ({nc}, {self.t}, {self.t})")
        return weights

    def solve(self, coef: np.ndarray, M: np.ndarray | None = None, return_info: bool = False,
              return_correctors: bool = False):
        """coef[N_c, n_el(, n_comp)] float64, M[N_c, d, d] or None -> A_eff[N_c, t, t] (and info[N_c]).

        With ``return_correctors`` the result is (A_eff, correctors[N_c, t, n^d * bs][, info]): the periodic cell solutions
        of the canonical loads (mean-free), dof = node * bs + component."""
        coef, nc = self._check_coef(coef)
        if return_correctors:
            corr = np.empty((nc, self.t, self.n_nodes * self._bs), dtype=np.float64)
            out, info = self._host_call("hommx_solve_batch_correctors", nc, M, lambda Mp, o, i: self._lib.hommx_solve_batch_correctors(
                self._h, nc, coef.ctypes.data, Mp, o, corr.ctypes.data, i))
            return (out, corr, info) if return_info else (out, corr)
        return self._host_call("hommx_solve_batch", nc, M, lambda Mp, o, i: self._lib.hommx_solve_batch(self._h, nc, coef.ctypes.data, Mp, o, i),
                               return_info)

    def _solve_stream(self, stream: CoefStream, M, return_info: bool):
        """The host solve of a coefficient in any form (hommx_solve_batch_source): what the three sampler methods below come to."""
        nc = self._check_stream(stream)
        src = stream.coef_source()
        return self._host_call("hommx_solve_batch_source", nc, M, lambda Mp, o, i: self._lib.hommx_solve_batch_source(
            self._h, nc, C.byref(src), Mp, o, i), return_info)

    def _check_stream(self, stream: CoefStream) -> int:
        """Shapes of a stream against the plan: the checks of ``solve``, ``solve_two_phase``, ``solve_separable`` and ``solve_program``;
        returns N_c."""
        nc = len(stream)
        if stream.method == "solve":
            return self._check_coef(stream.per_cell)[1]
        if stream.method == "solve_two_phase":
            if stream.shared[0].shape != (self.n_el,):
                raise ValueError(f"mask has shape {stream.shared[0].shape}; expected ({self.n_el},)")
            if stream.per_cell.size != nc * 2 * self.n_comp:
                raise ValueError(f"values has shape {stream.per_cell.shape}; expected ({nc}, 2" + (f", {self.n_comp})" if self.n_comp > 1 else ")"))
            return nc
        if stream.method == "solve_program":
            points, weights, prog = stream.shared
            if points.ndim != 3 or points.shape[0] != self.n_el or points.shape[2] != self.dim or points.shape[1] < 1:
                raise ValueError(f"points has shape {points.shape}; expected ({self.n_el}, n_q, {self.dim})")
            if weights.shape != (points.shape[1],):
                raise ValueError(f"weights must have shape ({points.shape[1]},)")
            if stream.per_cell.shape != (nc, 3 + prog.n_fields):
                raise ValueError(f"midpoints has shape {stream.per_cell.shape}; expected ({nc}, 3" + (
                    f" + {prog.n_fields}): the midpoint, then the fields" if prog.n_fields else ")"))
            if prog.n_comp != self.n_comp:
                raise ValueError(f"the expression has {prog.n_comp} components; the plan's coefficient has {self.n_comp}")
            return nc
        family, table, weights = stream.shared
        if family not in ("affine", "reciprocal"):
            raise KeyError(family)
        nq = 1 if family == "affine" else int(table.shape[1])
        if table.size != self.n_el * nq:
            raise ValueError(f"table has shape {table.shape}; expected ({self.n_el}" + (f", {nq})" if nq > 1 else ",)"))
        if family == "reciprocal" and (weights is None or weights.shape != (nq,)):
            raise ValueError(f"weights must have shape ({nq},)")
        want = (nc, 2) if self.n_comp == 1 else (nc, self.n_comp, 2)
        if stream.per_cell.shape != want:
            raise ValueError(f"params has shape {stream.per_cell.shape}; expected {want}")
        return nc

    def reconstruct(self, coef, xi: np.ndarray, M: np.ndarray | None = None, fields: bool = False, regions=None,
                    n_regions: int | None = None) -> Reconstruction:
        """HMM reconstruction: ``coef`` an array coef[N_c, n_el(, n_comp)] as ``solve`` takes it, or a ``CoefStream`` in any of its three
        forms (a sampler form sends a few numbers per cell and is expanded on the device: hommx_reconstruct_source); M as ``solve``,
        xi[N_c, t] the macro gradient / engineering-Voigt strain of every cell -> ``Reconstruction``; ``fields``: the per-element strain and
        flux [N_c, n_el, t] as well.  The correctors never leave the device; the batch runs in chunks of HOMMX_RECON_MEM_MB of correctors.

        ``regions``: integer labels [n_el] of the micro elements -> the ``region_*`` statistics over the elements of every label below
        ``n_regions`` (default: the largest label below 8, plus one); elements with any other label are in no region.  ``True`` with a
        two-phase stream: its mask is the labels (region 0: phase 0, region 1: phase 1)."""
        stream = self._as_stream(coef)
        nc = self._check_stream(stream)
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        if xi.shape != (nc, self.t):
            raise ValueError(f"xi has shape {xi.shape}; expected ({nc}, {self.t})")
        stats = np.empty((nc, 2 * self.t + 3), dtype=np.float64)
        strain = np.empty((nc, self.n_el, self.t), dtype=np.float64) if fields else None
        flux = np.empty((nc, self.n_el, self.t), dtype=np.float64) if fields else None
        sp, fp = (strain.ctypes.data, flux.ctypes.data) if fields else (None, None)
        labels, nr = None, 0
        if regions is True:
            if stream.method != "solve_two_phase":
                raise ValueError("regions=True takes the mask of a two-phase stream as the labels; pass labels for any other coefficient")
            nr = 2
        elif regions is not None:
            labels, nr = region_labels(regions, self.n_el, n_regions)
        rstats = np.empty((nc, nr, 2 * self.t + 4), dtype=np.float64) if nr else None
        src = stream.coef_source()
        A, info = self._host_call("hommx_reconstruct_source", nc, M, lambda Mp, o, i: self._lib.hommx_reconstruct_source(
            self._h, nc, C.byref(src), Mp, xi.ctypes.data, nr, None if labels is None else labels.ctypes.data, stats.ctypes.data,
            rstats.ctypes.data if nr else None, sp, fp, o, i))
        return Reconstruction.from_stats(xi, stats, A, info, strain, flux, region_stats=rstats)

    def sensitivities(self, coef, M: np.ndarray | None = None, directions=None, per_cell: bool = False, weights=None) -> Sensitivities:
        """Derivatives of A_H with respect to the micro coefficient (hommx_sensitivity_source): ``coef`` an array or a ``CoefStream`` and M
        as ``reconstruct`` takes them.  ``directions[n_dirs, n_el(, n_comp)]`` (shared by all cells) or, with ``per_cell``,
        ``directions[N_c, n_dirs, n_el(, n_comp)]``: up to 8 perturbations of one cell's element stream -> ``dA[N_c, n_dirs, t, t]`` =
        sum_K |K| s^m_K . material(dir_K) s^n_K, the derivative of A_H along each (the direction ``coef`` itself gives A_eff).
        ``weights[N_c, t, t]`` -> ``grad[N_c, n_el(, n_comp)]``, the gradient of weights : A_H with respect to every coefficient entry.
        At least one of the two.  The correctors never leave the device; the batch runs in the chunks of ``reconstruct``.
        ``directions="parameters"`` (``coef`` the program stream of an expression with parameters): the directions are the derivatives of
        the stream with respect to the parameters, formed on the device with the stream itself; ``dA[N_c, n_params, t, t]``."""
        stream = self._as_stream(coef)
        parameters = isinstance(directions, str) and directions == "parameters"
        nd, dirs = (self._parameter_count(coef), None) if parameters else (0, None)
        nc = self._check_stream(stream)
        if not parameters and directions is not None:
            dirs, nd = self._check_directions(directions, nc, per_cell)
        grad = None
        if weights is not None:
            weights = self._check_weights(weights, nc)
            grad = np.empty((nc,) + self._el, dtype=np.float64)
        elif nd == 0:
            raise ValueError("nothing requested: pass directions, weights or both")
        dA = np.empty((nc, nd, self.t, self.t), dtype=np.float64)
        args = _lib.SensArgs(nd, _per_cell_code(directions if parameters else per_cell), None if dirs is None else dirs.ctypes.data, dA.ctypes.data if nd else None,
                             None if grad is None else weights.ctypes.data, None if grad is None else grad.ctypes.data)
        A, info = self._source_call("hommx_sensitivity_source", nc, M, stream, args)
        return Sensitivities(dA, grad, A, info)

    def second_sensitivities(self, coef, M: np.ndarray | None = None, directions=None, per_cell: bool = False,
                             first: bool = False, curvature: bool = False) -> SecondSensitivities:
        """Second derivatives of A_H along coefficient directions (hommx_second_sensitivity_source): ``coef`` an array or a ``CoefStream``,
        M and ``directions`` (shared, or ``per_cell``) as ``sensitivities`` takes them -> ``d2A[N_c, n_dirs, n_dirs, t, t]``, exact on the
        discrete problem: the derivative of every canonical corrector along a direction is the corrector of a polarisation load, which the
        plan solves on the route ``load_kernel`` names (needs ``load_solve=True`` on the frontal mesh route).  ``first``: ``dA[N_c, n_dirs, t, t]`` of the same
        call as well.  One canonical pass and one load solve per direction; correctors and loads never leave the device; the batch runs in
        the chunks of ``reconstruct``.  ``directions="parameters"``: as in ``sensitivities``; d2A holds the second derivatives along the
        parameter tangents, which is the Hessian in the parameters when the expression is affine in them (``affine_in_parameters``).
        ``curvature=True`` (with ``directions="parameters"`` only): d2A also takes dA_H along the second derivatives of the stream
        (``expand_second_tangents``), formed on the device in the same pass -- the Hessian of A_H in the parameters and fields for any
        expression (HOMMX_DIRS_PARAMETERS_CURVATURE)"""
        stream = self._as_stream(coef)
        parameters = isinstance(directions, str) and directions == "parameters"
        code = _per_cell_code(directions if parameters else per_cell, curvature, "directions")
        nd, dirs = (self._parameter_count(coef), None) if parameters else (0, None)
        nc = self._check_stream(stream)
        if directions is None:
            raise ValueError("directions is required")
        if not parameters:
            dirs, nd = self._check_directions(directions, nc, per_cell)
        d2A = np.empty((nc, nd, nd, self.t, self.t), dtype=np.float64)
        dA = np.empty((nc, nd, self.t, self.t), dtype=np.float64) if first else None
        args = _lib.Sens2Args(nd, code, None if dirs is None else dirs.ctypes.data, d2A.ctypes.data, dA.ctypes.data if first else None)
        A, info = self._source_call("hommx_second_sensitivity_source", nc, M, stream, args)
        return SecondSensitivities(d2A, dA, A, info)

    def stratification_sensitivities(self, coef, M: np.ndarray | None = None, weights=None, full: bool = True) -> StratSensitivities:
        """Derivatives of A_H with respect to the stratification M (hommx_stratification_sensitivity_source): ``coef`` an array or a
        ``CoefStream`` and M as ``reconstruct`` takes them (without M: the derivative at M = I).  ``full`` -> ``dA_dM[N_c, d, d, t, t]``
        = dA_H[m, n] / dM[a, b]; ``weights[N_c, t, t]`` -> ``grad_M[N_c, d, d]`` = sum_mn weights[m, n] dA_dM[a, b, m, n], formed in one
        pass without the t x t intermediate.  At least one of the two.  The correctors never leave the device; the batch runs in the
        chunks of ``reconstruct``."""
        stream = self._as_stream(coef)
        nc = self._check_stream(stream)
        grad = None
        if weights is not None:
            weights = self._check_weights(weights, nc)
            grad = np.empty((nc, self.dim, self.dim), dtype=np.float64)
        elif not full:
            raise ValueError("nothing requested: pass weights, full=True or both")
        dA_dM = np.empty((nc, self.dim, self.dim, self.t, self.t), dtype=np.float64) if full else None
        args = _lib.StratSensArgs(dA_dM.ctypes.data if full else None, None if grad is None else weights.ctypes.data,
                                  None if grad is None else grad.ctypes.data)
        A, info = self._source_call("hommx_stratification_sensitivity_source", nc, M, stream, args)
        return StratSensitivities(dA_dM, grad, A, info)

    def _check_load_stream(self, P: CoefStream, nc: int):
        """Shapes of the program stream of a load (``CoefStream.program`` of a vector ``Expression``) against the plan."""
        if P.method != "solve_program":
            raise ValueError(f"a load given as a CoefStream must be CoefStream.program(...) of a vector Expression; got a {P.method!r} stream")
        points, weights, prog = P.shared
        if prog.n_comp != self.t:
            raise ValueError(f"the load expression has {prog.n_comp} components; a load of this plan has n_comp == t == {self.t}")
        if points.ndim != 3 or points.shape[0] != self.n_el or points.shape[2] != self.dim or points.shape[1] < 1:
            raise ValueError(f"points of the load has shape {points.shape}; expected ({self.n_el}, n_q, {self.dim})")
        if weights.shape != (points.shape[1],):
            raise ValueError(f"weights of the load must have shape ({points.shape[1]},)")
        if P.per_cell.shape != (nc, 3 + prog.n_fields):
            raise ValueError(f"the rows of the load have shape {P.per_cell.shape}; expected ({nc}, 3" + (
                f" + {prog.n_fields}): the midpoint, then the fields of the load expression" if prog.n_fields else ")"))

    def loads(self, coef, P, M: np.ndarray | None = None, per_cell: bool | None = None, response: bool = False, fields: bool = False,
              return_correctors: bool = False, eigenstrain: bool = False) -> LoadResponse:
        """User-supplied polarisation loads (hommx_loads_source): ``coef`` an array or a ``CoefStream`` and M as ``reconstruct`` takes them.
        ``P[n_loads, n_el, t]`` (shared by all cells) or ``P[N_c, n_loads, n_el, t]`` (``per_cell``, inferred from ``P.ndim`` when None):
        up to t prescribed flux / stress fields, constant per micro element, components in the order of ``Reconstruction.flux`` (shear not
        doubled) -> ``LoadResponse``.  ``P_eff`` comes from the canonical correctors alone on every plan; ``response`` adds a solve for the
        loads themselves (energy, mean / max total flux), ``fields`` the per-element strain and total flux of every load,
        ``return_correctors`` the load correctors (each implies ``response``; needs ``load_solve=True`` on the frontal mesh route).  The batch runs in the chunks
        of ``reconstruct``.

        ``P`` may also be a ``CoefStream.program(points, weights, ops, consts, t, rows, ...)`` built from a vector ``Expression`` with
        t components, the points and weights of a quadrature rule and the rows [N_c, 3 + n_fields] of the cells (HOMMX_LOADS_PROGRAM):
        ONE load, sampled on the device; only the rows cross per cell.  ``eigenstrain``: what ``P`` delivers -- array or program -- is
        an eigenstrain E in the components of ``Reconstruction.strain`` (shear DOUBLED), and the device forms the load
        ``-material(coef) E`` from the coefficient of the call (HOMMX_LOADS_EIGENSTRAIN)."""
        stream = self._as_stream(coef)
        nc = self._check_stream(stream)
        P_src = None
        if isinstance(P, CoefStream):
            self._check_load_stream(P, nc)
            P_src, nl, code, P_ptr = P.coef_source(), 1, _lib.LOADS_PROGRAM, None
        else:
            P = np.ascontiguousarray(P, dtype=np.float64)
            if per_cell is None:
                per_cell = P.ndim == 4
            lead = (nc,) if per_cell else ()
            nl = P.shape[len(lead)] if P.ndim == len(lead) + 3 else -1
            if nl < 0 or P.shape != lead + (nl, self.n_el, self.t):
                raise ValueError(f"P has shape {P.shape}; expected {lead + ('n_loads', self.n_el, self.t)}")
            if not 1 <= nl <= self.t:
                raise ValueError(f"n_loads must be 1 .. {self.t}; got {nl}")
            code, P_ptr = int(bool(per_cell)), P.ctypes.data
        if eigenstrain:
            code |= _lib.LOADS_EIGENSTRAIN
        response = bool(response or fields or return_correctors)
        P_eff = np.empty((nc, nl, self.t), dtype=np.float64)
        energy = np.empty((nc, nl, nl), dtype=np.float64) if response else None
        stats = np.empty((nc, nl, self.t + 2), dtype=np.float64) if response else None
        strain = np.empty((nc, nl, self.n_el, self.t), dtype=np.float64) if fields else None
        flux = np.empty((nc, nl, self.n_el, self.t), dtype=np.float64) if fields else None
        corr = np.empty((nc, nl, self.n_nodes * self._bs), dtype=np.float64) if return_correctors else None
        addr = lambda a: None if a is None else a.ctypes.data
        args = _lib.LoadArgs(nl, code, P_ptr, P_eff.ctypes.data, None, addr(energy), addr(stats), addr(strain), addr(flux),
                             addr(corr), None, C.pointer(P_src) if P_src is not None else None)
        A, info = self._source_call("hommx_loads_source", nc, M, stream, args)
        r = LoadResponse(P_eff, A, info, energy, strain=strain, flux=flux, correctors=corr)
        if response:
            r.mean_flux, r.max_flux = stats[:, :, :self.t].copy(), stats[:, :, self.t].copy()
            r.argmax_element = stats[:, :, self.t + 1].astype(np.int64)
        return r

    def _criterion_program(self, crit, n_history: int | None = None) -> Program:
        """The program of a ``hommx_amd.expr.Criterion`` on this plan (its index checks against t and n_comp run here); ``n_history``:
        the history variables of the law whose state it is evaluated on (None: a criterion of the linear state)."""
        if n_history is None and crit.reads_state:
            names = ", ".join(f"{n}[{crit.state_indices[n] - 1}]" for n in "bh" if crit.state_indices[n])
            raise ValueError(f"the criterion reads {names}, the nonlinear state: it is evaluated behind the secant iteration "
                             "(secant(criterion=...), criterion(nonlinear=True) of the solver classes)")
        ops, consts = crit.program(self.t, self.n_comp) if n_history is None else crit.program(self.t, self.n_comp, n_history)
        if crit.n_y > self.dim:
            raise ValueError(f"the criterion reads y[{crit.n_y - 1}]; the micro mesh has {self.dim} dimensions")
        return Program(np.ascontiguousarray(ops), np.ascontiguousarray(consts), 1, int(crit.n_params), int(crit.n_fields))

    def criterion(self, coef, xi: np.ndarray, crit, M: np.ndarray | None = None, rows=None, points=None, values: bool = False,
                  fields: bool = False, P=None, per_cell: bool | None = None, eigenstrain: bool = False) -> CriterionResult:
        """A failure criterion on the reconstructed micro state (hommx_criterion_source): ``coef`` an array or a ``CoefStream``, xi and M
        as ``reconstruct`` takes them, ``crit`` a ``hommx_amd.expr.Criterion`` -> ``CriterionResult``: per cell the largest value, the
        element reaching it, the mean and the volume fraction at or above ``crit.threshold``.  The stress never leaves the device:
        four numbers per macro cell come back, unless ``values`` (v_K of every element) or ``fields`` (the strain and flux the
        criterion saw) ask for more.  ``rows[N_c, 3 + crit.n_fields]``: the macro midpoint and the criterion's own fields of every cell
        (required when the criterion reads ``f``; without them ``x`` is 0); ``points[n_el, dim]``: the element centroids, required when
        it reads ``y``.

        ``P``: ONE load as ``loads`` takes it -- ``P[n_el, t]`` / ``P[1, n_el, t]`` shared by all cells, ``P[N_c, (1,) n_el, t]`` per
        cell, or a program ``CoefStream`` of a vector ``Expression``; ``eigenstrain`` as in ``loads``.  The criterion then sees the
        total state, strain xi + eps(chi^xi + chi_P) and flux material . strain + P, after a load solve on the route ``load_kernel``
        names (needs ``load_solve=True`` on the frontal mesh route).  The batch runs in the chunks of ``reconstruct`` / ``loads``."""
        stream = self._as_stream(coef)
        nc = self._check_stream(stream)
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        if xi.shape != (nc, self.t):
            raise ValueError(f"xi has shape {xi.shape}; expected ({nc}, {self.t})")
        prog = self._criterion_program(crit)
        pstruct = prog.struct()
        if rows is None:
            if crit.n_fields:
                raise ValueError(f"the criterion reads the fields {', '.join(crit.field_names)}: pass rows[N_c, 3 + {crit.n_fields}]")
            rows = np.zeros((nc, 3))
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.shape != (nc, 3 + crit.n_fields):
            raise ValueError(f"rows has shape {rows.shape}; expected ({nc}, 3 + {crit.n_fields}): the midpoint, then the criterion's fields")
        if points is not None:
            points = np.ascontiguousarray(points, dtype=np.float64)
            if points.shape != (self.n_el, self.dim):
                raise ValueError(f"points has shape {points.shape}; expected ({self.n_el}, {self.dim}): the element centroids")
        elif crit.n_y:
            raise ValueError(f"the criterion reads y[{crit.n_y - 1}]: pass points[n_el, dim], the element centroids")
        P, P_src, P_ptr, code = self._one_load(P, per_cell, eigenstrain, nc)
        out = np.empty((nc, _lib.CRIT_NSTATS), dtype=np.float64)
        vals = np.empty((nc, self.n_el), dtype=np.float64) if values else None
        strain = np.empty((nc, self.n_el, self.t), dtype=np.float64) if fields else None
        flux = np.empty((nc, self.n_el, self.t), dtype=np.float64) if fields else None
        addr = lambda a: None if a is None else a.ctypes.data
        args = _lib.CriterionArgs(C.pointer(pstruct), int(crit.n_fields), rows.ctypes.data, addr(points), xi.ctypes.data, float(crit.threshold),
                                  int(P is not None), code, P_ptr, C.pointer(P_src) if P_src is not None else None, out.ctypes.data,
                                  addr(vals), addr(strain), addr(flux), None, None)
        A, info = self._source_call("hommx_criterion_source", nc, M, stream, args)
        return CriterionResult(out[:, 0].copy(), out[:, 1].astype(np.int64), out[:, 2].copy(), out[:, 3].copy(), A, info, vals, strain, flux)

    def _one_load(self, P, per_cell, eigenstrain, nc: int) -> tuple:
        """ONE load of ``criterion`` / ``secant`` as the library takes it -> (P, P_source, P_ptr, code): a program ``CoefStream`` gives
        its source and LOADS_PROGRAM; an array -- ``P[n_el, t]`` / ``P[1, n_el, t]`` shared (repeated for every cell: ``points`` is
        the call's one shared array), ``P[N_c, (1,) n_el, t]`` per cell -- the contiguous ``P[N_c, n_el, t]``, its address and
        LOADS_PER_CELL; None gives (None, None, None, 0).  ``eigenstrain`` sets the flag of a load that is there."""
        P_src, P_ptr, code = None, None, 0
        if isinstance(P, CoefStream):
            self._check_load_stream(P, nc)
            P_src, code = P.coef_source(), _lib.LOADS_PROGRAM
        elif P is not None:
            P = np.asarray(P, dtype=np.float64)
            if P.ndim == 4 and P.shape[1] == 1:  # per cell, with the axis of the one load
                P = P[:, 0]
            elif P.ndim == 3 and P.shape[0] == 1 and not per_cell:  # shared, with that axis
                P = P[0]
            if P.shape not in ((self.n_el, self.t), (nc, self.n_el, self.t)):
                raise ValueError(f"P has shape {P.shape}; expected ({self.n_el}, {self.t}) or ({nc}, {self.n_el}, {self.t}), one load "
                                 "(an axis of length 1 for it is accepted)")
            P = np.ascontiguousarray(np.broadcast_to(P, (nc, self.n_el, self.t)))  # a shared load is repeated: points is the call's shared array
            P_ptr, code = P.ctypes.data, _lib.LOADS_PER_CELL
        if eigenstrain and P is not None:
            code |= _lib.LOADS_EIGENSTRAIN
        return P, P_src, P_ptr, code

    def _law_program(self, law) -> Program:
        """The program of a ``hommx_amd.expr.SecantLaw`` on this plan (its component count and index checks against t and n_comp run here)."""
        ops, consts = law.program(self.t, self.n_comp)
        if law.n_y > self.dim:
            raise ValueError(f"the law reads y[{law.n_y - 1}]; the micro mesh has {self.dim} dimensions")
        return Program(np.ascontiguousarray(ops), np.ascontiguousarray(consts), self.n_comp + int(law.n_history), int(law.n_params),
                       int(law.n_fields))

    def _law_history(self, law, history, nc: int) -> np.ndarray | None:
        """``history`` of ``secant`` / ``secant_tangent`` as float64[nc, n_el, n_history] (a copy), or None for a law without history
        variables: [N, n_el, n_history], [N, n_el] for one variable, or a scalar / [n_history] broadcast as an initial state."""
        nh = int(law.n_history)
        if not nh:
            if history is not None:
                raise ValueError("the law has no history variables: history must be None")
            return None
        want = f"history[N_c, n_el, n_history] = ({nc}, {self.n_el}, {nh})" + (f", ({nc}, {self.n_el})" if nh == 1 else "") + \
            f", a scalar or ({nh},) values as the initial state of every element"
        if history is None:
            raise ValueError(f"the law has the history variables {', '.join(law.history_names)}: pass {want}")
        h = np.asarray(history, dtype=np.float64)
        if h.shape == (nc, self.n_el) and nh == 1:
            h = h[:, :, None]
        elif h.shape in ((), (1,), (nh,)):
            h = np.broadcast_to(h.reshape(-1), (nc, self.n_el, nh))
        elif h.shape != (nc, self.n_el, nh):
            raise ValueError(f"history has shape {h.shape}; expected {want}")
        return np.array(h, dtype=np.float64, order="C")

    @staticmethod
    def _secant_limits(max_iter, tol, relax) -> tuple[int, float, float]:
        max_iter, tol, relax = int(max_iter), float(tol), float(relax)
        if max_iter < 1:
            raise ValueError(f"max_iter must be at least 1; got {max_iter}")
        if not tol >= 0.0:
            raise ValueError(f"tol must be a number >= 0; got {tol}")
        if not 0.0 < relax <= 1.0:
            raise ValueError(f"relax must lie in (0, 1]; got {relax}")
        return max_iter, tol, relax

    def secant(self, coef, xi: np.ndarray, law, M: np.ndarray | None = None, rows=None, points=None, max_iter: int = 50, tol: float = 1e-10,
               relax: float = 1.0, coef_start=None, fields: bool = False, values: bool = False, return_coef: bool = False,
               history=None, P=None, per_cell: bool | None = None, eigenstrain: bool = False, criterion=None, crit_rows=None,
               crit_values: bool = False, crit_fields: bool = False, reconstruct: bool = False, regions=None,
               n_regions: int | None = None) -> SecantResult:
        """The secant iteration of a strain-dependent coefficient (hommx_secant_source): ``coef`` an array or a ``CoefStream``, the BASE
        coefficient ``c`` of the law; xi and M as ``reconstruct`` takes them; ``law`` a ``hommx_amd.expr.SecantLaw`` with the plan's
        ``n_comp`` components -> ``SecantResult``.  Per cell and round: the correctors of the current stream on the plan's route, the
        strain and the secant flux of every element, the law on them, the relaxed candidate ``(1 - relax) c + relax v``; the cell stops
        when the largest change relative to the largest entry is at most ``tol``, after ``max_iter`` rounds, on a value that is not
        finite or on a flagged pivot, and what comes back is the state of that round.  The element fields never leave the device
        unless ``fields`` / ``values`` / ``return_coef`` ask for them.  ``rows[N_c, 3 + law.n_fields]``: the macro midpoint and the
        law's own fields of every cell (required when the law reads ``f``; without them ``x`` is 0); ``points[n_el, dim]``: the
        element centroids, required when it reads ``y``; ``coef_start[N_c, n_el(, n_comp)]``: the stream the iteration starts from
        (default: the base stream), e.g. ``SecantResult.coef`` of a neighbouring macro strain.  The batch runs in the chunks of
        ``reconstruct``.

        ``history``: required for a law with history variables (hommx_secant_history_source) -- what ``h[k]`` reads, the
        state at the start of the call, frozen for the whole iteration: ``[N_c, n_el, n_history]``, ``[N_c, n_el]`` for one variable,
        or a scalar / ``[n_history]`` values broadcast as an initial state.  ``SecantResult.history`` is then the update of every
        element at its cell's stopping round; the argument is not changed.  ``ValueError`` naming the expected shape otherwise.

        ``P``: ONE load beside the law (hommx_secant_load_source), with the meaning ``criterion`` gives ``P``,
        ``per_cell`` and ``eigenstrain``: an array ``[N_c, n_el, t]`` (or one ``[n_el, t]`` for all cells) or a program ``CoefStream``
        of a vector ``Expression``.  Every round then ends in a load solve on the current stream (the route ``load_kernel`` names;
        ``load_solve=True`` on the frontal mesh route).  A polarisation: the law reads the total strain in ``e`` and the total flux
        ``material . e + P`` in ``s``.  An eigenstrain: it reads the elastic strain ``e - E`` and ``material . (e - E)``, the model
        sigma = c(eps - eps*) (eps - eps*).  ``strain`` / ``flux`` are what the law read, ``mean_flux`` the mean of that flux, and the
        effective polarisation of the stopping state is ``mean_flux - A_eff xi``.  With ``P=None`` the call is the one it was.

        ``criterion`` / ``reconstruct``: a tail on the state every cell stops in (hommx_secant_state_source), without
        another elimination and without the stream leaving the device.  ``criterion``: a ``hommx_amd.expr.Criterion``, which may read
        ``b[k]`` (the base coefficient) and, declared with ``history=law.n_history``, ``h[k]`` (``history`` of this call) beside what
        ``MicroCellPlan.criterion`` gives it; ``c[k]`` is the stream the iteration stopped on and ``e`` / ``s`` the TOTAL strain and
        flux (``material . e + P``, P the polarisation or the eigenstress).  ``crit_rows[N_c, 3 + criterion.n_fields]``: the
        criterion's own rows (default: the midpoints of ``rows``; required when it reads ``f``); ``crit_values`` / ``crit_fields``:
        ``values`` / ``strain`` and ``flux`` of the ``CriterionResult``.  ``reconstruct`` (with ``regions`` / ``n_regions`` as
        ``reconstruct`` takes them; not together with ``P``: the statistics have no load term) -> ``SecantResult.reconstruction``.
        For a criterion that reads neither ``b`` nor ``h`` the results are bit for bit ``criterion(result.coef, ...)`` /
        ``reconstruct(result.coef, ...)``.  With none of them the call is the one it was."""
        tail = None
        if criterion is not None or reconstruct:
            tail = (criterion, crit_rows, bool(crit_values), bool(crit_fields), bool(reconstruct), regions, n_regions)
        elif crit_rows is not None or crit_values or crit_fields or regions is not None:
            raise ValueError("crit_rows / crit_values / crit_fields belong to criterion=..., regions to reconstruct=True")
        return self._secant(coef, xi, law, M, rows, points, max_iter, tol, relax, coef_start, fields, values, return_coef, history=history,
                            load=(P, per_cell, eigenstrain), tail=tail)

    def _state_tail(self, tail, law, stream, nc: int, rows, points, loaded: bool) -> tuple:
        """The tail of ``secant`` as the library takes it -> (hommx_secant_state_args, what keeps its arrays alive, finish), where
        ``finish(xi, A_eff, info)`` gives (``CriterionResult`` or None, ``Reconstruction`` or None) once the call has returned."""
        crit, crit_rows, want_values, want_fields, recon, regions, n_regions = tail
        addr = lambda a: None if a is None else a.ctypes.data
        keep, sargs = [], _lib.SecantStateArgs()
        out = vals = strain = flux = stats = rstats = None
        if crit is not None:
            prog = self._criterion_program(crit, int(law.n_history))
            pstruct = prog.struct()
            if crit_rows is None:
                if crit.n_fields:
                    raise ValueError(f"the criterion reads the fields {', '.join(crit.field_names)}: pass crit_rows[N_c, 3 + {crit.n_fields}]")
                crit_rows = rows[:, :3]
            crit_rows = np.ascontiguousarray(crit_rows, dtype=np.float64)
            if crit_rows.shape != (nc, 3 + crit.n_fields):
                raise ValueError(f"crit_rows has shape {crit_rows.shape}; expected ({nc}, 3 + {crit.n_fields}): the midpoint, then the "
                                 "criterion's fields")
            if crit.n_y and points is None:
                raise ValueError(f"the criterion reads y[{crit.n_y - 1}]: pass points[n_el, dim], the element centroids")
            out = np.empty((nc, _lib.CRIT_NSTATS), dtype=np.float64)
            vals = np.empty((nc, self.n_el), dtype=np.float64) if want_values else None
            strain = np.empty((nc, self.n_el, self.t), dtype=np.float64) if want_fields else None
            flux = np.empty((nc, self.n_el, self.t), dtype=np.float64) if want_fields else None
            sargs.crit_program, sargs.crit_n_fields, sargs.crit_rows = C.pointer(pstruct), int(crit.n_fields), crit_rows.ctypes.data
            sargs.threshold, sargs.crit, sargs.crit_values = float(crit.threshold), out.ctypes.data, addr(vals)
            sargs.total_strain, sargs.total_flux = addr(strain), addr(flux)
            keep += [prog, pstruct, crit_rows]
        elif crit_rows is not None or want_values or want_fields:
            raise ValueError("crit_rows / crit_values / crit_fields belong to criterion=...")
        if recon:
            if loaded:
                raise ValueError("reconstruct=True together with a load P: the reconstruction statistics have no load term; ask for "
                                 "criterion=..., crit_fields=True, which returns the loaded state")
            labels, nr = None, 0
            if regions is True:
                if stream.method != "solve_two_phase":
                    raise ValueError("regions=True takes the mask of a two-phase stream as the labels; pass labels for any other coefficient")
                nr = 2
            elif regions is not None:
                labels, nr = region_labels(regions, self.n_el, n_regions)
            stats = np.empty((nc, 2 * self.t + 3), dtype=np.float64)
            rstats = np.empty((nc, nr, 2 * self.t + 4), dtype=np.float64) if nr else None
            sargs.reconstruct, sargs.n_regions, sargs.region = 1, nr, addr(labels)
            sargs.stats, sargs.region_stats = stats.ctypes.data, addr(rstats)
            keep += [labels]
        elif regions is not None:
            raise ValueError("regions belong to reconstruct=True")

        def finish(xi, A, info):
            c = None if out is None else CriterionResult(out[:, 0].copy(), out[:, 1].astype(np.int64), out[:, 2].copy(), out[:, 3].copy(),
                                                         A, info, vals, strain, flux)
            r = None if stats is None else Reconstruction.from_stats(xi, stats, A, info, region_stats=rstats)
            return c, r

        return sargs, keep, finish

    @property
    def tangent_kind(self) -> str:
        """The kind of the sibling plan ``secant_tangent`` eliminates the tangent coefficient on: a full symmetric t x t matrix per
        element -- "poisson_matrix" for the Poisson kinds, "elasticity_voigt" for the elasticity kinds."""
        return "poisson_matrix" if self.kind.startswith("poisson") else "elasticity_voigt"

    def _check_tangent(self, law, tangent_plan):
        """What ``secant_tangent`` and ``secant_tangent_device`` refuse before the library does: an implicit law, a sibling plan of the
        wrong kind or shape."""
        if not law.explicit:
            raise ValueError(f"the law reads s[{law.state_indices['s'] - 1}]: the consistent tangent takes an explicit law, one that reads no "
                             "s[k]; an implicit law is out of scope")
        if not isinstance(tangent_plan, MicroCellPlan) or tangent_plan is self:
            raise ValueError(f"tangent_plan must be another MicroCellPlan, of kind {self.tangent_kind!r} on the same micro mesh")
        if tangent_plan.kind != self.tangent_kind:
            raise ValueError(f"tangent_plan has kind {tangent_plan.kind!r}; the tangent kind of a {self.kind!r} plan is {self.tangent_kind!r}")
        mine, its = (self.dim, self.n_micro, self.n_el, self.n_nodes, self.device), \
            (tangent_plan.dim, tangent_plan.n_micro, tangent_plan.n_el, tangent_plan.n_nodes, tangent_plan.device)
        if mine != its:
            raise ValueError(f"tangent_plan has (dim, n_micro, n_el, n_nodes, device) = {its}; the plan has {mine}")

    def secant_tangent(self, coef, xi: np.ndarray, law, tangent_plan: "MicroCellPlan", M: np.ndarray | None = None, rows=None, points=None,
                       max_iter: int = 50, tol: float = 1e-10, relax: float = 1.0, coef_start=None, fields: bool = False,
                       values: bool = False, return_coef: bool = False, return_tangent_coef: bool = False, history=None, P=None,
                       per_cell: bool | None = None, eigenstrain: bool = False) -> SecantResult:
        """``secant`` and, at the state every cell stops in, the consistent tangent D = d mean_flux / d xi (hommx_secant_tangent_source;
        DESIGN 4.16): the arguments of ``secant`` and ``tangent_plan``, a plan of ``self.tangent_kind`` on the same micro mesh and
        device (``MicroCellPlan(dim, n, plan.tangent_kind)`` or ``from_mesh`` of the same mesh).  Every member ``secant`` returns has
        its bits; ``tangent``, ``asymmetry``, ``tangent_info`` and, with ``return_tangent_coef``, ``tangent_coef`` come with them.
        The law must be explicit (``law.explicit``): ``ValueError`` naming the ``s[k]`` it reads otherwise, and for a ``tangent_plan``
        of the wrong kind or shape.  ``history``: as in ``secant`` (hommx_secant_tangent_history_source); the tangent is that of the
        components at the frozen history, so a cell that unloads has ``tangent`` = ``A_eff``.  ``P``, ``per_cell``, ``eigenstrain``:
        the load of ``secant`` (hommx_secant_tangent_load_source); the element tangents are then evaluated at the strain the law
        read, total or elastic, and ``tangent`` is still d mean_flux / d xi."""
        self._check_tangent(law, tangent_plan)
        return self._secant(coef, xi, law, M, rows, points, max_iter, tol, relax, coef_start, fields, values, return_coef, tangent_plan,
                            return_tangent_coef, history, (P, per_cell, eigenstrain))

    def _secant(self, coef, xi, law, M, rows, points, max_iter, tol, relax, coef_start, fields, values, return_coef, tangent_plan=None,
                return_tangent_coef=False, history=None, load=(None, None, False), tail=None) -> SecantResult:
        """The host call of ``secant`` (``tangent_plan`` None) and ``secant_tangent``, on the entry ``_secant_entry`` names for what the
        call has: a history (a law with history variables), a load (``load`` = (P, per_cell, eigenstrain) with a P), a tail (``tail``:
        what ``secant`` asks for on the stopped state)."""
        stream = self._as_stream(coef)
        nc = self._check_stream(stream)
        P, P_src, P_ptr, code = self._one_load(load[0], load[1], load[2], nc)
        largs = None if P is None else _lib.SecantLoadArgs(code, P_ptr, C.pointer(P_src) if P_src is not None else None)
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        if xi.shape != (nc, self.t):
            raise ValueError(f"xi has shape {xi.shape}; expected ({nc}, {self.t})")
        max_iter, tol, relax = self._secant_limits(max_iter, tol, relax)
        prog = self._law_program(law)
        pstruct = prog.struct()
        hist_in = self._law_history(law, history, nc)
        hist_out = None if hist_in is None else np.empty_like(hist_in)
        hargs = None if hist_in is None else _lib.HistoryArgs(int(law.n_history), hist_in.ctypes.data, hist_out.ctypes.data)
        if rows is None:
            if law.n_fields:
                raise ValueError(f"the law reads the fields {', '.join(law.field_names)}: pass rows[N_c, 3 + {law.n_fields}]")
            rows = np.zeros((nc, 3))
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.shape != (nc, 3 + law.n_fields):
            raise ValueError(f"rows has shape {rows.shape}; expected ({nc}, 3 + {law.n_fields}): the midpoint, then the law's fields")
        if points is not None:
            points = np.ascontiguousarray(points, dtype=np.float64)
            if points.shape != (self.n_el, self.dim):
                raise ValueError(f"points has shape {points.shape}; expected ({self.n_el}, {self.dim}): the element centroids")
        elif law.n_y:
            raise ValueError(f"the law reads y[{law.n_y - 1}]: pass points[n_el, dim], the element centroids")
        el = self._el
        if coef_start is not None:
            coef_start = np.ascontiguousarray(coef_start, dtype=np.float64)
            if coef_start.shape != (nc,) + el:
                raise ValueError(f"coef_start has shape {coef_start.shape}; expected {(nc,) + el}")
        state = np.empty((nc, _lib.SECANT_NSTATE), dtype=np.float64)
        mean_flux = np.empty((nc, self.t), dtype=np.float64)
        out_coef = np.empty((nc,) + el, dtype=np.float64) if return_coef else None
        strain = np.empty((nc, self.n_el, self.t), dtype=np.float64) if fields else None
        flux = np.empty((nc, self.n_el, self.t), dtype=np.float64) if fields else None
        vals = np.empty((nc, self.n_el, self.n_comp), dtype=np.float64) if values else None
        addr = lambda a: None if a is None else a.ctypes.data
        args = _lib.SecantArgs(C.pointer(pstruct), int(law.n_fields), rows.ctypes.data, addr(points), xi.ctypes.data, max_iter, tol, relax,
                               addr(coef_start), state.ctypes.data, None, mean_flux.ctypes.data, addr(out_coef), addr(strain), addr(flux),
                               addr(vals), None)
        sargs = finish = None
        if tail is not None:
            if tangent_plan is not None:
                raise ValueError("a tail behind the tangent entries is out of scope: call secant(criterion=...) for the state")
            sargs, keep, finish = self._state_tail(tail, law, stream, nc, rows, points, largs is not None)
        struct, D, asym, tinfo, tcoef = args, None, None, None, None
        if tangent_plan is not None:
            D = np.empty((nc, self.t, self.t), dtype=np.float64)
            asym = np.empty(nc, dtype=np.float64)
            tinfo = np.zeros(nc, dtype=np.int32)
            tcoef = np.empty((nc, self.n_el, self.t * (self.t + 1) // 2), dtype=np.float64) if return_tangent_coef else None
            struct = _lib.SecantTangentArgs(C.pointer(args), tangent_plan._h, D.ctypes.data, asym.ctypes.data, addr(tcoef), tinfo.ctypes.data)
        what, more = _secant_entry(tangent_plan is not None, hargs, largs, sargs, device=False)
        src = stream.coef_source()

        def call(Mp, o, i):
            args.A_eff, args.info = o, i
            return getattr(self._lib, what)(self._h, nc, C.byref(src), Mp, C.byref(struct), *more)

        A, info = self._host_call(what, nc, M, call)
        crit_result, recon_result = (None, None) if finish is None else finish(xi, A, info)
        return SecantResult(A_eff=A, mean_flux=mean_flux, rounds=state[:, 0].astype(np.int64), change=state[:, 1].copy(),
                            status=state[:, 2].astype(np.int64), info=info, coef=out_coef, strain=strain, flux=flux, values=vals, tangent=D,
                            asymmetry=asym, tangent_info=tinfo, tangent_coef=tcoef, history=hist_out, criterion=crit_result,
                            reconstruction=recon_result)

    def solve_two_phase(self, mask: np.ndarray, values: np.ndarray, M: np.ndarray | None = None,
                        return_info: bool = False):
        """Two-phase media sampled on the device: mask[n_el] (bool / uint8, phase of every micro element) and
        values[N_c, 2(, n_comp)] = coefficient of phase 0 / phase 1 at every macro cell -> A_eff[N_c, t, t]."""
        return self._solve_stream(CoefStream.two_phase(mask, values), M, return_info)

    def solve_separable(self, family: str, table: np.ndarray, weights: np.ndarray | None, params: np.ndarray,
                        M: np.ndarray | None = None, return_info: bool = False):
        """Separable coefficient sampled on the device (include/hommx_hip.h): ``family`` "affine" (table[n_el] = element means of
        g) or "reciprocal" (table[n_el, n_q] = g at the quadrature points, weights[n_q]); params[N_c, 2] = (a, b) per macro cell."""
        return self._solve_stream(CoefStream.separable(family, table, weights, params), M, return_info)

    def solve_program(self, points: np.ndarray, weights: np.ndarray, program: Program, midpoints: np.ndarray, M: np.ndarray | None = None,
                      return_info: bool = False):
        """Expression coefficient sampled on the device (include/hommx_hip.h, HOMMX_COEF_PROGRAM): points[n_el, n_q, dim] and
        weights[n_q] of the micro quadrature rule, the program, midpoints[N_c, 3 + program.n_fields] of the macro cells -> A_eff[N_c, t, t]."""
        stream = CoefStream("solve_program", (np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(weights, dtype=np.float64), program),
                            np.ascontiguousarray(midpoints, dtype=np.float64))
        return self._solve_stream(stream, M, return_info)

    def expand(self, stream: CoefStream) -> np.ndarray:
        """The element stream coef[N_c, n_el(, n_comp)] the library expands ``stream`` to on the device (hommx_expand_source): what
        ``solve`` would be given.  A program's stream equals ``Expression.host_stream`` bit for bit for exactly rounded operations."""
        return self._expand("hommx_expand_source", stream)[0]

    def _expand(self, what: str, stream: CoefStream, *slots: int) -> tuple:
        """Check ``stream``, allocate coef[N_c, n_el(, n_comp)] and one array [N_c, k, n_el(, n_comp)] for every k of ``slots``, and run the
        host entry point ``what``(plan, N_c, source, outputs...) unless the batch is empty."""
        nc = self._check_stream(stream)
        outs = tuple(np.empty((nc,) + lead + self._el, dtype=np.float64) for lead in [()] + [(k,) for k in slots])
        if nc:
            src = stream.coef_source()
            _lib.check(getattr(self._lib, what)(self._h, nc, C.byref(src), *(o.ctypes.data for o in outs)), what)
        return outs

    def expand_tangents(self, stream: CoefStream) -> tuple[np.ndarray, np.ndarray]:
        """(coef[N_c, n_el(, n_comp)], dirs[N_c, n_params + n_fields, n_el(, n_comp)]) of the program stream of an expression with
        parameters or fields (hommx_expand_tangents): the stream of ``expand``, bit for bit, and its derivatives with respect to the
        parameters, then the fields (of a cell: its own value), formed in one
        forward-mode pass on the device.  dirs equals ``Expression.host_tangents`` bit for bit for exactly rounded operations."""
        return self._expand("hommx_expand_tangents", stream, self._parameter_count(stream))

    def expand_second_tangents(self, stream: CoefStream) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(coef, dirs, curv[N_c, n_pairs, n_el(, n_comp)]) of the program stream of an expression with parameters or fields
        (hommx_expand_second_tangents): coef and dirs are those of ``expand_tangents``, bit for bit, and curv the second derivatives of
        the stream with respect to the pairs (a, b), a <= b, of the differentiable slots in the order of ``Expression.pairs``, formed
        in one second-order forward-mode pass on the device (one per pair of slots for 3 or 4 slots).  curv equals
        ``Expression.host_second_tangents`` bit for bit for exactly rounded operations."""
        n_tan = self._parameter_count(stream)
        return self._expand("hommx_expand_second_tangents", stream, n_tan, n_tan * (n_tan + 1) // 2)

    # -- device pointers (torch tensors or raw ints), asynchronous --------------------------------
    def expand_second_tangents_device(self, n_cells: int, source: "_lib.CoefSource", coef_ptr: int | None, dirs_ptr: int | None, curv_ptr: int,
                                      stream: int | None = None):
        """Device-pointer form of ``expand_second_tangents`` (hommx_expand_second_tangents_device), asynchronous on ``stream``;
        ``coef_ptr`` / ``dirs_ptr`` None: not written."""
        _lib.check(self._lib.hommx_expand_second_tangents_device(self._h, int(n_cells), C.byref(source), coef_ptr or None, dirs_ptr or None,
                                                                 curv_ptr, stream or None), "hommx_expand_second_tangents_device")

    def expand_tangents_device(self, n_cells: int, source: "_lib.CoefSource", coef_ptr: int | None, dirs_ptr: int, stream: int | None = None):
        """Device-pointer form of ``expand_tangents`` (hommx_expand_tangents_device), asynchronous on ``stream``; ``coef_ptr`` None: the
        tangents alone."""
        _lib.check(self._lib.hommx_expand_tangents_device(self._h, int(n_cells), C.byref(source), coef_ptr or None, dirs_ptr, stream or None),
                   "hommx_expand_tangents_device")

    def solve_source_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, out_ptr: int, info_ptr: int | None,
                            stream: int | None = None):
        """Device-pointer solve of a coefficient in any form (hommx_solve_batch_source_device), asynchronous on ``stream``: ``source`` =
        ``CoefStream.coef_source(upload)`` with device addresses."""
        _lib.check(self._lib.hommx_solve_batch_source_device(self._h, int(n_cells), C.byref(source), M_ptr or None, out_ptr, info_ptr or None,
                                                             stream or None), "hommx_solve_batch_source_device")

    def expand_device(self, n_cells: int, source: "_lib.CoefSource", out_ptr: int, stream: int | None = None):
        """Device-pointer form of ``expand`` (hommx_expand_source_device), asynchronous on ``stream``."""
        _lib.check(self._lib.hommx_expand_source_device(self._h, int(n_cells), C.byref(source), out_ptr, stream or None),
                   "hommx_expand_source_device")

    def solve_program_device(self, n_cells: int, points_ptr: int, weights_ptr: int, n_q: int, program: Program, midpoints_ptr: int,
                             M_ptr: int | None, out_ptr: int, info_ptr: int | None, stream: int | None = None):
        """Device twin of ``solve_program``: the points, weights and midpoints are device pointers, the program stays host memory."""
        prog = program.struct()
        src = _lib.CoefSource(form=_lib.COEF_PROGRAM, n_q=int(n_q), n_fields=int(program.n_fields), table=points_ptr, weights=weights_ptr,
                              params=midpoints_ptr, program=C.pointer(prog))
        self.solve_source_device(n_cells, src, M_ptr, out_ptr, info_ptr, stream)

    def reconstruct_device(self, n_cells: int, coef_ptr: int, M_ptr: int | None, xi_ptr: int, stats_ptr: int, strain_ptr: int | None = None,
                           flux_ptr: int | None = None, A_ptr: int | None = None, info_ptr: int | None = None, stream: int | None = None):
        """Device-pointer form of ``reconstruct`` (hommx_reconstruct_batch_device), asynchronous on ``stream``: stats[n_cells, 2t + 3] =
        [mean_strain | mean_flux | energy | max_flux | argmax_element]."""
        _lib.check(
            self._lib.hommx_reconstruct_batch_device(self._h, int(n_cells), coef_ptr, M_ptr or None, xi_ptr, stats_ptr, strain_ptr or None,
                                                     flux_ptr or None, A_ptr or None, info_ptr or None, stream or None),
            "hommx_reconstruct_batch_device",
        )

    def reconstruct_source_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, xi_ptr: int, stats_ptr: int,
                                  n_regions: int = 0, region_ptr: int | None = None, region_stats_ptr: int | None = None,
                                  strain_ptr: int | None = None, flux_ptr: int | None = None, A_ptr: int | None = None,
                                  info_ptr: int | None = None, stream: int | None = None):
        """Device-pointer form of ``reconstruct`` for any coefficient form (hommx_reconstruct_source_device), asynchronous on ``stream``:
        ``source`` = ``CoefStream.coef_source(upload)`` with device addresses; region_stats[n_cells, n_regions, 2t + 4] =
        [volume | sums (not divided) | max | argmax]; a two-phase source with ``n_regions`` 2 and no ``region_ptr`` takes its mask."""
        _lib.check(
            self._lib.hommx_reconstruct_source_device(self._h, int(n_cells), C.byref(source), M_ptr or None, xi_ptr, int(n_regions),
                                                      region_ptr or None, stats_ptr, region_stats_ptr or None, strain_ptr or None,
                                                      flux_ptr or None, A_ptr or None, info_ptr or None, stream or None),
            "hommx_reconstruct_source_device",
        )

    def sensitivities_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, n_dirs: int = 0, dirs_ptr: int | None = None,
                             per_cell: bool = False, dA_ptr: int | None = None, weights_ptr: int | None = None, grad_ptr: int | None = None,
                             A_ptr: int | None = None, info_ptr: int | None = None, stream: int | None = None):
        """Device-pointer form of ``sensitivities`` (hommx_sensitivity_source_device), asynchronous on ``stream``: ``source`` =
        ``CoefStream.coef_source(upload)`` with device addresses; dirs[n_dirs, n_el, n_comp] or, ``per_cell``, [n_cells, n_dirs, n_el, n_comp]
        -> dA[n_cells, n_dirs, t, t]; weights[n_cells, t, t] -> grad[n_cells, n_el, n_comp].  ``per_cell="parameters"``: the directions
        are the parameter tangents of the source's program (no ``dirs_ptr``, ``n_dirs`` its n_params)."""
        args = _lib.SensArgs(int(n_dirs), _per_cell_code(per_cell), dirs_ptr or None, dA_ptr or None, weights_ptr or None, grad_ptr or None,
                             A_ptr or None, info_ptr or None)
        _lib.check(self._lib.hommx_sensitivity_source_device(self._h, int(n_cells), C.byref(source), M_ptr or None, C.byref(args), stream or None),
                   "hommx_sensitivity_source_device")

    def second_sensitivities_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, n_dirs: int, dirs_ptr: int, d2A_ptr: int,
                                    per_cell: bool = False, dA_ptr: int | None = None, A_ptr: int | None = None, info_ptr: int | None = None,
                                    stream: int | None = None, curvature: bool = False):
        """Device-pointer form of ``second_sensitivities`` (hommx_second_sensitivity_source_device), asynchronous on ``stream``: ``source`` =
        ``CoefStream.coef_source(upload)`` with device addresses; dirs[n_dirs, n_el, n_comp] or, ``per_cell``, [n_cells, n_dirs, n_el, n_comp]
        -> d2A[n_cells, n_dirs, n_dirs, t, t]; dA[n_cells, n_dirs, t, t] on request.  ``per_cell="parameters"``: as in
        ``sensitivities_device``; with ``curvature=True`` d2A takes the curvature term as well (HOMMX_DIRS_PARAMETERS_CURVATURE)."""
        args = _lib.Sens2Args(int(n_dirs), _per_cell_code(per_cell, curvature), dirs_ptr or None, d2A_ptr or None, dA_ptr or None, A_ptr or None, info_ptr or None)
        _lib.check(self._lib.hommx_second_sensitivity_source_device(self._h, int(n_cells), C.byref(source), M_ptr or None, C.byref(args),
                                                                    stream or None),
                   "hommx_second_sensitivity_source_device")

    def stratification_sensitivities_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, dA_dM_ptr: int | None = None,
                                            weights_ptr: int | None = None, grad_M_ptr: int | None = None, A_ptr: int | None = None,
                                            info_ptr: int | None = None, stream: int | None = None):
        """Device-pointer form of ``stratification_sensitivities`` (hommx_stratification_sensitivity_source_device), asynchronous on
        ``stream``: ``source`` = ``CoefStream.coef_source(upload)`` with device addresses; dA_dM[n_cells, d, d, t, t];
        weights[n_cells, t, t] -> grad_M[n_cells, d, d]."""
        args = _lib.StratSensArgs(dA_dM_ptr or None, weights_ptr or None, grad_M_ptr or None, A_ptr or None, info_ptr or None)
        _lib.check(self._lib.hommx_stratification_sensitivity_source_device(self._h, int(n_cells), C.byref(source), M_ptr or None, C.byref(args),
                                                                            stream or None),
                   "hommx_stratification_sensitivity_source_device")

    def loads_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, n_loads: int, P_ptr: int, P_eff_ptr: int,
                     per_cell: bool = False, A_ptr: int | None = None, info_ptr: int | None = None, energy_ptr: int | None = None,
                     stats_ptr: int | None = None, strain_ptr: int | None = None, flux_ptr: int | None = None,
                     correctors_ptr: int | None = None, stream: int | None = None, eigenstrain: bool = False,
                     P_source: "_lib.CoefSource | None" = None):
        """Device-pointer form of ``loads`` (hommx_loads_source_device), asynchronous on ``stream``: ``source`` =
        ``CoefStream.coef_source(upload)`` with device addresses; P[n_loads, n_el, t] or, ``per_cell``, [n_cells, n_loads, n_el, t] ->
        P_eff[n_cells, n_loads, t]; energy[n_cells, n_loads, n_loads], stats[n_cells, n_loads, t + 2] = [mean total flux | max | argmax],
        strain / flux[n_cells, n_loads, n_el, t] and correctors[n_cells, n_loads, n_nodes * bs]: any of them triggers the load solve.
        ``P_source``: the load comes from a program instead (HOMMX_LOADS_PROGRAM) -- ``CoefStream.program(...).coef_source(upload)`` of a
        vector ``Expression`` with t components; ``P_ptr`` and ``per_cell`` are then not read and ``n_loads`` must be 1.
        ``eigenstrain``: the array or the program delivers an eigenstrain (HOMMX_LOADS_EIGENSTRAIN), as ``loads`` describes."""
        code = _lib.LOADS_PROGRAM if P_source is not None else int(bool(per_cell))
        if eigenstrain:
            code |= _lib.LOADS_EIGENSTRAIN
        args = _lib.LoadArgs(int(n_loads), code, None if P_source is not None else P_ptr, P_eff_ptr, A_ptr or None, energy_ptr or None,
                             stats_ptr or None, strain_ptr or None, flux_ptr or None, correctors_ptr or None, info_ptr or None,
                             C.pointer(P_source) if P_source is not None else None)
        _lib.check(self._lib.hommx_loads_source_device(self._h, int(n_cells), C.byref(source), M_ptr or None, C.byref(args), stream or None),
                   "hommx_loads_source_device")

    def criterion_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, xi_ptr: int, crit, rows_ptr: int, crit_ptr: int,
                         points_ptr: int | None = None, values_ptr: int | None = None, strain_ptr: int | None = None,
                         flux_ptr: int | None = None, P_ptr: int | None = None, P_source: "_lib.CoefSource | None" = None,
                         eigenstrain: bool = False, A_ptr: int | None = None, info_ptr: int | None = None, stream: int | None = None):
        """Device-pointer form of ``criterion`` (hommx_criterion_source_device), asynchronous on ``stream``: ``source`` =
        ``CoefStream.coef_source(upload)`` with device addresses; ``crit`` the ``Criterion`` (its program is host memory);
        rows[n_cells, 3 + crit.n_fields], points[n_el, dim] (None: the criterion reads no ``y``) -> crit[n_cells, 4] = [max | argmax
        element | sum |K| v | sum |K| [v >= threshold]], values[n_cells, n_el], strain / flux[n_cells, n_el, t].  A load:
        ``P_ptr`` (P[n_cells, n_el, t], per cell) or ``P_source`` (a program, as in ``loads_device``), ``eigenstrain`` as there."""
        prog = self._criterion_program(crit)
        pstruct = prog.struct()
        has_load = P_ptr is not None or P_source is not None
        code = (_lib.LOADS_PROGRAM if P_source is not None else _lib.LOADS_PER_CELL) | (_lib.LOADS_EIGENSTRAIN if eigenstrain else 0)
        args = _lib.CriterionArgs(C.pointer(pstruct), int(crit.n_fields), rows_ptr, points_ptr or None, xi_ptr, float(crit.threshold),
                                  int(has_load), code if has_load else 0, None if P_source is not None else P_ptr or None,
                                  C.pointer(P_source) if P_source is not None else None, crit_ptr, values_ptr or None, strain_ptr or None,
                                  flux_ptr or None, A_ptr or None, info_ptr or None)
        _lib.check(self._lib.hommx_criterion_source_device(self._h, int(n_cells), C.byref(source), M_ptr or None, C.byref(args), stream or None),
                   "hommx_criterion_source_device")

    def secant_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, xi_ptr: int, law, rows_ptr: int, state_ptr: int,
                      A_ptr: int, points_ptr: int | None = None, max_iter: int = 50, tol: float = 1e-10, relax: float = 1.0,
                      coef_start_ptr: int | None = None, mean_flux_ptr: int | None = None, coef_ptr: int | None = None,
                      strain_ptr: int | None = None, flux_ptr: int | None = None, values_ptr: int | None = None, info_ptr: int | None = None,
                      stream: int | None = None, history_in_ptr: int | None = None, history_out_ptr: int | None = None,
                      P_ptr: int | None = None, P_source: "_lib.CoefSource | None" = None, eigenstrain: bool = False, criterion=None,
                      crit_rows_ptr: int | None = None, crit_ptr: int | None = None, crit_values_ptr: int | None = None,
                      total_strain_ptr: int | None = None, total_flux_ptr: int | None = None, stats_ptr: int | None = None,
                      n_regions: int = 0, regions_ptr: int | None = None, region_stats_ptr: int | None = None):
        """Device-pointer form of ``secant`` (hommx_secant_source_device), asynchronous on ``stream``: ``source`` =
        ``CoefStream.coef_source(upload)`` with device addresses; ``law`` the ``SecantLaw`` (its program is host memory);
        rows[n_cells, 3 + law.n_fields], points[n_el, dim] (None: the law reads no ``y``) -> state[n_cells, 3] = [rounds | change |
        status] (doubles), A_eff[n_cells, t, t], mean_flux[n_cells, t], coef[n_cells, n_el, n_comp] (the stream A_eff belongs to),
        strain / flux[n_cells, n_el, t], values[n_cells, n_el, n_comp].  Exactly ``max_iter`` rounds per chunk are queued and nothing
        is read back; the bits are those of ``secant``.  A law with history variables (hommx_secant_history_source_device) takes
        ``history_in_ptr`` and ``history_out_ptr``, two different arrays [n_cells, n_el, n_history] on the device: a caller keeps the
        history resident by swapping them between load steps.  A load beside the law (hommx_secant_load_source_device): ``P_ptr``
        (P[n_cells, n_el, t], per cell) or ``P_source`` (a program, as in ``loads_device``), ``eigenstrain`` as in ``secant``; an
        eigenstrain array is read in every round and never written.

        The tail on the stopped state (hommx_secant_state_source_device), queued behind the ``max_iter`` rounds:
        ``criterion`` (a ``Criterion``, as in ``secant``) with crit_rows[n_cells, 3 + criterion.n_fields] -> crit[n_cells, 4],
        crit_values[n_cells, n_el], total_strain / total_flux[n_cells, n_el, t]; ``stats_ptr``: the reconstruction statistics
        stats[n_cells, 2 t + 3] and, with ``n_regions``, regions[n_el] (uint8) -> region_stats[n_cells, n_regions, 2 t + 4]."""
        args, hargs, largs, keep = self._device_args(law, (max_iter, tol, relax), (history_in_ptr, history_out_ptr),
                                                     (P_ptr, P_source, eigenstrain), rows_ptr, points_ptr, xi_ptr, coef_start_ptr, state_ptr,
                                                     A_ptr, mean_flux_ptr, coef_ptr, strain_ptr, flux_ptr, values_ptr, info_ptr)
        sargs = None
        if criterion is not None or stats_ptr:
            sargs = _lib.SecantStateArgs()
            if criterion is not None:
                if not crit_rows_ptr or not crit_ptr:
                    raise ValueError("criterion=... takes crit_rows_ptr and crit_ptr")
                cprog = self._criterion_program(criterion, int(law.n_history))
                cstruct = cprog.struct()
                sargs.crit_program, sargs.crit_n_fields, sargs.crit_rows = C.pointer(cstruct), int(criterion.n_fields), crit_rows_ptr
                sargs.threshold, sargs.crit, sargs.crit_values = float(criterion.threshold), crit_ptr, crit_values_ptr or None
                sargs.total_strain, sargs.total_flux = total_strain_ptr or None, total_flux_ptr or None
            if stats_ptr:
                sargs.reconstruct, sargs.n_regions, sargs.region = 1, int(n_regions), regions_ptr or None
                sargs.stats, sargs.region_stats = stats_ptr, region_stats_ptr or None
        elif crit_rows_ptr or crit_ptr or crit_values_ptr or total_strain_ptr or total_flux_ptr or regions_ptr or region_stats_ptr or n_regions:
            raise ValueError("the crit_* pointers belong to criterion=..., the regions to stats_ptr")
        self._secant_device_call(n_cells, source, M_ptr, args, False, hargs, largs, sargs, stream)

    def _device_args(self, law, limits, history, load, rows_ptr, points_ptr, xi_ptr, coef_start_ptr, state_ptr, A_ptr, *optional) -> tuple:
        """What ``secant_device`` and ``secant_tangent_device`` build alike -> (``SecantArgs``, ``HistoryArgs`` or None,
        ``SecantLoadArgs`` or None, what keeps the program alive): ``limits`` = (max_iter, tol, relax), ``history`` = (history_in_ptr,
        history_out_ptr), ``load`` = (P_ptr, P_source, eigenstrain), ``optional`` = the pointers behind A_eff in the struct's order."""
        hargs = self._device_history(law, *history)
        max_iter, tol, relax = self._secant_limits(*limits)
        prog = self._law_program(law)
        pstruct = prog.struct()
        args = _lib.SecantArgs(C.pointer(pstruct), int(law.n_fields), rows_ptr, points_ptr or None, xi_ptr, max_iter, tol, relax,
                               coef_start_ptr or None, state_ptr, A_ptr, *(q or None for q in optional))
        return args, hargs, self._device_load(*load), (prog, pstruct)

    def _secant_device_call(self, n_cells, source, M_ptr, struct, tangent: bool, hargs, largs, sargs, stream):
        """The device entry of the combination (``_secant_entry``) on ``struct``, the ``SecantArgs`` or ``SecantTangentArgs`` of the call."""
        what, more = _secant_entry(tangent, hargs, largs, sargs, device=True)
        _lib.check(getattr(self._lib, what)(self._h, int(n_cells), C.byref(source), M_ptr or None, C.byref(struct), *more, stream or None), what)

    @staticmethod
    def _device_load(P_ptr, P_source, eigenstrain):
        """The ``SecantLoadArgs`` of a device call, None without a load."""
        if P_ptr is None and P_source is None:
            return None
        code = (_lib.LOADS_PROGRAM if P_source is not None else _lib.LOADS_PER_CELL) | (_lib.LOADS_EIGENSTRAIN if eigenstrain else 0)
        return _lib.SecantLoadArgs(code, None if P_source is not None else P_ptr, C.pointer(P_source) if P_source is not None else None)

    @staticmethod
    def _device_history(law, history_in_ptr, history_out_ptr):
        """The ``HistoryArgs`` of a device call, None for a law without history variables; ``ValueError`` for pointers that do not go
        with the law."""
        if not law.n_history:
            if history_in_ptr or history_out_ptr:
                raise ValueError("the law has no history variables: history_in_ptr and history_out_ptr must be None")
            return None
        if not history_in_ptr or not history_out_ptr or history_in_ptr == history_out_ptr:
            raise ValueError(f"the law has the history variables {', '.join(law.history_names)}: pass history_in_ptr and history_out_ptr, two "
                             f"different device arrays [n_cells, n_el, {law.n_history}]")
        return _lib.HistoryArgs(int(law.n_history), history_in_ptr, history_out_ptr)

    def secant_tangent_device(self, n_cells: int, source: "_lib.CoefSource", M_ptr: int | None, xi_ptr: int, law,
                              tangent_plan: "MicroCellPlan", rows_ptr: int, state_ptr: int, A_ptr: int, tangent_ptr: int, asymmetry_ptr: int,
                              points_ptr: int | None = None, max_iter: int = 50, tol: float = 1e-10, relax: float = 1.0,
                              coef_start_ptr: int | None = None, mean_flux_ptr: int | None = None, coef_ptr: int | None = None,
                              strain_ptr: int | None = None, flux_ptr: int | None = None, values_ptr: int | None = None,
                              info_ptr: int | None = None, tangent_coef_ptr: int | None = None, tangent_info_ptr: int | None = None,
                              stream: int | None = None, history_in_ptr: int | None = None, history_out_ptr: int | None = None,
                              P_ptr: int | None = None, P_source: "_lib.CoefSource | None" = None, eigenstrain: bool = False):
        """Device-pointer form of ``secant_tangent`` (hommx_secant_tangent_source_device), asynchronous on ``stream``: the pointers of
        ``secant_device`` and tangent[n_cells, t, t], asymmetry[n_cells], tangent_coef[n_cells, n_el, t (t + 1) / 2],
        tangent_info[n_cells] (int32).  Per chunk ``max_iter`` rounds, one tangent launch and one solve on ``tangent_plan`` are queued
        and nothing is read back; the bits are those of ``secant_tangent``.  ``history_in_ptr`` / ``history_out_ptr``: as in
        ``secant_device`` (hommx_secant_tangent_history_source_device); ``P_ptr`` / ``P_source`` / ``eigenstrain``: the load of
        ``secant_device`` (hommx_secant_tangent_load_source_device)."""
        self._check_tangent(law, tangent_plan)
        args, hargs, largs, keep = self._device_args(law, (max_iter, tol, relax), (history_in_ptr, history_out_ptr),
                                                     (P_ptr, P_source, eigenstrain), rows_ptr, points_ptr, xi_ptr, coef_start_ptr, state_ptr,
                                                     A_ptr, mean_flux_ptr, coef_ptr, strain_ptr, flux_ptr, values_ptr, info_ptr)
        targs = _lib.SecantTangentArgs(C.pointer(args), tangent_plan._h, tangent_ptr, asymmetry_ptr, tangent_coef_ptr or None,
                                       tangent_info_ptr or None)
        self._secant_device_call(n_cells, source, M_ptr, targs, True, hargs, largs, None, stream)

    def solve_separable_device(self, n_cells: int, family: str, n_q: int, table_ptr: int, weights_ptr: int | None, params_ptr: int,
                               M_ptr: int | None, out_ptr: int, info_ptr: int | None, stream: int | None = None):
        fam = {"affine": _lib.SAMPLER_AFFINE, "reciprocal": _lib.SAMPLER_RECIPROCAL}[family]
        _lib.check(
            self._lib.hommx_solve_batch_separable_device(self._h, int(n_cells), fam, int(n_q), table_ptr, weights_ptr or None, params_ptr,
                                                         M_ptr or None, out_ptr, info_ptr or None, stream or None),
            "hommx_solve_batch_separable_device",
        )

    def solve_two_phase_device(self, n_cells: int, mask_ptr: int, values_ptr: int, M_ptr: int | None, out_ptr: int,
                               info_ptr: int | None, stream: int | None = None):
        _lib.check(
            self._lib.hommx_solve_batch_two_phase_device(
                self._h, int(n_cells), mask_ptr, values_ptr, M_ptr or None, out_ptr, info_ptr or None, stream or None
            ),
            "hommx_solve_batch_two_phase_device",
        )

    def solve_device(self, n_cells: int, coef_ptr: int, M_ptr: int | None, out_ptr: int, info_ptr: int | None,
                     stream: int | None = None):
        _lib.check(
            self._lib.hommx_solve_batch_device(
                self._h, int(n_cells), coef_ptr, M_ptr or None, out_ptr, info_ptr or None, stream or None
            ),
            "hommx_solve_batch_device",
        )
