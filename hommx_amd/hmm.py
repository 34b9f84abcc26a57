"""HMM solver classes with the constructor / ``solve()`` surface of flxrcz/hommx (``src/hommx/hmm.py``), driving the
batched HIP micro-cell solver instead of the per-cell DOLFINx/PETSc loop.

What is kept from the reference:
  * class names, constructor argument order, ``solve()``, ``set_boundary_conditions``, ``set_right_hand_side``,
    ``function_space`` (hmm.py:63-73, 173-176, 276-296, 434; class signatures :561-571, :717-728, :843-853, :976-987);
  * the log-don't-raise error convention (hmm.py:320-323, 427-430) and the ``_needs_reassembly`` cache (hmm.py:150, 287, 300-301, 332);
  * default homogeneous Dirichlet conditions for ``PoissonHMM`` (hmm.py:598-636), none for elasticity (hmm.py:806-807);
  * the macro algorithm of ``solve()`` (hmm.py:434-491): assemble, lift Dirichlet values bc by bc, zero rows+columns, solve.
What differs (DOLFINx/UFL/PETSc are not dependencies):
  * meshes are ``hommx_amd.mesh.Mesh``; ``A(x, y)``, ``f(x)``, ``Dtheta_transpose(x)`` are NumPy-vectorised callables
    (x: the cell midpoint, 3 components as the ``fem.Constant`` of hmm.py:190-192; y: array [dim, npts]);
  * the micro problems of ALL macro cells are solved in one batched GPU call (``_assemble_stiffness``);
  * the macro system is solved with a sparse direct solver (SciPy); ``petsc_options_*`` are accepted for signature
    compatibility and are advisory (a direct solve has no tolerance; the reference's own tightest test also uses LU,
    test_integration_poisson.py:207-212).
The micro solves have NO CPU path in this package: without the HIP library / a GPU, ``solve()`` raises.
"""

from __future__ import annotations

import dataclasses
import logging
from abc import ABC, abstractmethod
from collections.abc import Callable

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import fem
from .batch import (CoefStream, CriterionResult, LoadResponse, MicroCellPlan, Reconstruction, SecantResult, SecondSensitivities,
                    Sensitivities, StratSensitivities, region_labels)
from .expr import Criterion, Expression, SecantLaw
from .mesh import Mesh, micro_cells_per_side

_VOIGT = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]}


def _join(parts: list, **override):
    """The results of the chunks of a batch (one of the result dataclasses of ``batch``) as one: every field concatenated along the
    cells, a field that is None staying None, the fields of ``override`` as given (what the chunks do not know: ``cells``, ``names``)."""
    def cat(name):
        first = getattr(parts[0], name)
        if first is None:
            return None
        if dataclasses.is_dataclass(first):  # a result inside a result: the tail of a SecantResult
            return _join([getattr(r, name) for r in parts])
        return np.concatenate([getattr(r, name) for r in parts])

    return type(parts[0])(**{f.name: override[f.name] if f.name in override else cat(f.name) for f in dataclasses.fields(parts[0])})


def _unroll_dofs(dofs: np.ndarray, bs: int) -> np.ndarray:
    """hmm.py:31-40."""
    dofs = np.asarray(dofs)
    if bs == 1:
        return dofs
    return (dofs[..., None] * bs + np.arange(bs)).reshape(dofs.shape[:-1] + (-1,))


def micro_quadrature(dim: int, degree: int):
    """Barycentric points / weights of the rule that samples the coefficient: degree <= 1 centroid; 2: 3 / 4
    points; 3: 6-point Strang-Fix (triangle), 8-point collapsed Gauss-Jacobi (tetrahedron: positive weights -- the classical
    5-point Keast rule has a weight of -0.8 and can turn the element mean of a high-contrast coefficient non-positive; Basix's
    own 6-point Xiao-Gimbutas rule is not available offline: parity unpinned for that rule)."""
    import itertools

    if degree <= 1:
        return np.full((1, dim + 1), 1.0 / (dim + 1)), np.ones(1)
    if dim == 2 and degree == 2:
        p = np.full((3, 3), 1.0 / 6.0)
        np.fill_diagonal(p, 2.0 / 3.0)
        return p, np.full(3, 1.0 / 3.0)
    if dim == 2 and degree == 3:
        a, b, c = 0.659027622374092, 0.231933368553031, 0.109039009072877
        return np.array(list(itertools.permutations((a, b, c)))), np.full(6, 1.0 / 6.0)
    if dim == 3 and degree == 2:
        a, b = 0.5854101966249685, 0.1381966011250105
        p = np.full((4, 4), b)
        np.fill_diagonal(p, a)
        return p, np.full(4, 0.25)
    return fem.simplex_quadrature(dim, degree)


def hooke_to_voigt(C: np.ndarray, dim: int) -> np.ndarray:
    """[..., d,d,d,d] -> [..., t, t] with Cv[m][n] = E^m : C : E^n for the tensorial unit strains E^m."""
    pairs = _VOIGT[dim]
    t = len(pairs)
    out = np.empty(C.shape[:-4] + (t, t))
    for m, (i, j) in enumerate(pairs):
        for n, (k, l) in enumerate(pairs):
            out[..., m, n] = 0.25 * (C[..., i, j, k, l] + C[..., j, i, k, l] + C[..., i, j, l, k] + C[..., j, i, l, k])
    return out


def material_matrix(coef: np.ndarray, kind: str, dim: int) -> np.ndarray:
    """[..., t, t]: the material matrix of element means ``coef[...(, n_comp)]`` in the layout of the plan kind ``kind``, in the basis
    of the canonical loads (Poisson: A; elasticity: ``hooke_to_voigt`` of the Hooke tensor) -- the host statement of ``material()`` in
    csrc/mesh_elem.h."""
    coef = np.asarray(coef, dtype=float)
    t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
    if kind == "poisson":
        return coef[..., None, None] * np.eye(t)
    C = np.zeros(coef.shape[:-1] + (t, t))
    if kind == "poisson_matrix":
        for c, (i, j) in enumerate(_VOIGT[dim]):
            C[..., i, j] = C[..., j, i] = coef[..., c]
    elif kind == "elasticity":
        lam, mu = coef[..., 0], coef[..., 1]
        C[..., :dim, :dim] = lam[..., None, None]
        for m in range(t):
            C[..., m, m] += 2.0 * mu if m < dim else mu
    else:  # the upper triangle of the t x t matrix, row-major
        iu = np.triu_indices(t)
        C[..., iu[0], iu[1]] = coef
        C[..., iu[1], iu[0]] = coef
    return C


def eigenstress(coef: np.ndarray, kind: str, dim: int, E: np.ndarray) -> np.ndarray:
    """P = -material(coef) E: the polarisation of an eigenstrain ``E[..., t]`` (the components of ``Reconstruction.strain``, shear
    doubled) on elements of the coefficient ``coef`` (``material_matrix``); the leading axes broadcast."""
    return -np.einsum("...mn,...n->...m", material_matrix(coef, kind, dim), np.asarray(E, dtype=float))


class Lame:
    """Isotropic Hooke tensor given by its Lame parameters: ``A = lambda d_ij d_kl + mu (d_ik d_jl + d_il d_jk)``
    (test_integration_linear_elasticity.py:84-93; rotated_fibers.py:66-76).  Returning ``Lame(lam, mu)`` from the
    coefficient callable selects the 2-component isotropic kernel instead of the 21-component Voigt one."""

    def __init__(self, lam, mu):
        self.lam, self.mu = lam, mu


def _lame_stacked(v: Lame, shape: tuple) -> np.ndarray:
    """[shape..., 2] = (lambda, mu), each broadcast to ``shape``: the layout the sampling takes an isotropic coefficient in."""
    return np.stack([np.broadcast_to(np.asarray(v.lam, float), shape), np.broadcast_to(np.asarray(v.mu, float), shape)], axis=-1)


class TwoPhase:
    """Two-phase coefficient  A(x, y) = inside(x) if indicator(y) else outside(x)  -- the shape of every coefficient in the
    reference's examples (laminate.py:101-102, inclusion.py:107-118, rotated_fibers.py:23-38: ``ufl.conditional`` of the
    fast variable between two values).  Passing one as ``A`` lets the solver classes sample on the DEVICE: the phase mask is
    evaluated once on the micro mesh (element barycentres: UFL estimates degree 0 for a conditional, i.e. the centroid rule)
    and two values per macro cell are sent instead of n_el samples (``hommx_solve_batch_two_phase``).

    ``indicator(y)``: y[dim, npts] -> bool[npts];  ``inside(x)`` / ``outside(x)``: x[3, N_c] -> scalar, [N_c] array, or a
    ``Lame`` of such (elasticity).  The object is also a plain callable ``A(x, y)``, so every generic path accepts it.
    """

    def __init__(self, indicator, inside, outside):
        self.indicator, self.inside, self.outside = indicator, inside, outside

    @staticmethod
    def _pair(v, n):
        if isinstance(v, Lame):
            return np.stack([np.broadcast_to(np.asarray(v.lam, float), (n,)), np.broadcast_to(np.asarray(v.mu, float), (n,))], axis=-1)
        return np.broadcast_to(np.asarray(v, float), (n,))

    def phase_values(self, c: np.ndarray) -> np.ndarray:
        """[N_c, 2(, 2)]: (outside, inside) at the macro cell midpoints c[N_c, 3]."""
        n = c.shape[0]
        return np.stack([self._pair(self.outside(c.T), n), self._pair(self.inside(c.T), n)], axis=1)

    def __call__(self, x, y):
        m = np.asarray(self.indicator(y), dtype=bool)
        vin, vout = self.inside(x), self.outside(x)
        if isinstance(vin, Lame):
            return Lame(np.where(m, vin.lam, vout.lam), np.where(m, vin.mu, vout.mu))
        return np.where(m, vin, vout)


class Separable:
    """Separable scalar coefficient  A(x, y) = a(x) + b(x) g(y)  (``family="affine"``)  or  1 / (a(x) + b(x) g(y))
    (``family="reciprocal"``) -- the shape of the smooth coefficients in the reference's own tests
    (test_integration_poisson.py:124-125  1/(2 + cos 2 pi y0);  :149-150, 197  0.33 + 0.15 (sin 2 pi x0 + sin 2 pi y0);
    :268  1.1 + x0 + sin 2 pi y0).  Passing one as ``A`` of a Poisson solver class lets it sample on the DEVICE
    (``hommx_solve_batch_separable``): g is tabulated once on the micro mesh at the points of the degree-3 rule UFL would
    pick, and two numbers per macro cell cross the boundary instead of n_el samples.

    ``a(x)`` / ``b(x)``: x[3, N_c] -> scalar or [N_c];  ``g(y)``: y[dim, npts] -> [npts].  For the elasticity classes ``a`` / ``b`` return
    ``Lame(lam, mu)`` (affine family): lambda = a.lam + b.lam g, mu = a.mu + b.mu g -- the isotropic Hooke tensor of the reference's 2D
    beam test, lambda = 1.25, mu = 5 + 4.5 sin 2 pi y0 (test_integration_linear_elasticity.py:78-93).  The object is also a plain
    callable ``A(x, y)``.  ``host_stream`` is the documented host equivalent of the device sampler: the same IEEE operations in the
    same order, hence the same bits (tests/test_gpu_separable.py)."""

    def __init__(self, family: str, a, b, g, degree: int = 3):
        """``degree``: quadrature degree of the rule that samples g -- 3 is UFL's estimate for ONE transcendental function of
        the fast variable (sin 2 pi y0: 1 + 2), the shape of every smooth coefficient in the reference's tests."""
        if family not in ("affine", "reciprocal"):
            raise ValueError("family must be 'affine' or 'reciprocal'")
        self.family, self.a, self.b, self.g, self.degree = family, a, b, g, int(degree)

    def params(self, c: np.ndarray) -> np.ndarray:
        """[N_c, 2] = (a, b) at the macro cell midpoints c[N_c, 3]; [N_c, 2, 2] = ((a, b) of lambda, (a, b) of mu) when a / b return ``Lame``."""
        n = c.shape[0]
        a, b = self.a(c.T), self.b(c.T)
        bc = lambda v: np.broadcast_to(np.asarray(v, float), (n,))
        if isinstance(a, Lame) or isinstance(b, Lame):
            a = a if isinstance(a, Lame) else Lame(a, a)
            b = b if isinstance(b, Lame) else Lame(b, b)
            return np.stack([np.stack([bc(a.lam), bc(b.lam)], axis=1), np.stack([bc(a.mu), bc(b.mu)], axis=1)], axis=1)
        return np.stack([bc(a), bc(b)], axis=1)

    def table(self, yq: np.ndarray, w: np.ndarray) -> np.ndarray:
        """yq[n_el, n_q, dim] -> what the C ABI takes: affine: element means of g [n_el]; reciprocal: g at the points [n_el, n_q]."""
        n_el, nq, d = yq.shape
        gq = np.asarray(self.g(yq.reshape(-1, d).T), float).reshape(n_el, nq)
        if self.family == "affine":
            acc = np.zeros(n_el)
            for q in range(nq):
                acc = acc + w[q] * gq[:, q]
            return acc
        return gq

    def host_stream(self, params: np.ndarray, table: np.ndarray, w: np.ndarray) -> np.ndarray:
        """Element means coef[N_c, n_el(, 2)] exactly as the device sampler forms them."""
        if params.ndim == 3:  # one (a, b) pair per Lame parameter
            return np.stack([self.host_stream(params[:, k], table, w) for k in range(params.shape[1])], axis=-1)
        a, b = params[:, 0:1], params[:, 1:2]
        if self.family == "affine":
            return a + b * table[None, :]
        acc = np.zeros((params.shape[0], table.shape[0]))
        for q in range(table.shape[1]):
            acc = acc + w[q] * (1.0 / (a + b * table[None, :, q]))
        return acc

    def __call__(self, x, y):
        a, b, g = self.a(x), self.b(x), self.g(y)
        if isinstance(a, Lame) or isinstance(b, Lame):
            if self.family != "affine":
                raise ValueError("Lame-valued Separable coefficients are affine (lambda, mu = a + b g)")
            a = a if isinstance(a, Lame) else Lame(a, a)
            b = b if isinstance(b, Lame) else Lame(b, b)
            return Lame(a.lam + b.lam * g, a.mu + b.mu * g)
        v = a + b * g
        return v if self.family == "affine" else 1.0 / v


def isotropic_hooke(lam, mu, dim: int) -> np.ndarray:
    lam, mu = np.asarray(lam, float), np.asarray(mu, float)
    I = np.eye(dim)
    t1 = np.einsum("ij,kl->ijkl", I, I)
    t2 = np.einsum("ik,jl->ijkl", I, I) + np.einsum("il,jk->ijkl", I, I)
    return lam[..., None, None, None, None] * t1 + mu[..., None, None, None, None] * t2


class BaseHMM(ABC):
    """hmm.py:53-511."""

    _kind = "poisson"

    def __init__(
        self,
        msh: Mesh,
        A: Callable,
        f: Callable,
        msh_micro: Mesh,
        eps: float,
        petsc_options_global_solve: dict | None = None,
        petsc_options_cell_problem: dict | None = None,
        petsc_options_prefix: str = "hommx_HMM",
        *,
        quadrature_degree: int | None = None,
        rhs_quadrature_degree: int = 6,
        device: int | None = None,
        reserve: bool = False,
        tree_loads: bool = False,
    ):
        """``quadrature_degree``: degree of the micro quadrature rule that samples ``A(x, .)``.  The reference lets UFL estimate it
        from the expression (hmm.py:190-198 + fem.form at :644-647): 0 for a ``conditional`` between constants, 3 for one
        transcendental function of the fast variable -- ``sin(2 pi y0)``, ``1/(2 + cos(2 pi y0))``: the coefficients of its own
        tests (test_integration_poisson.py:124-125, 149-150, 197).  A Python callable has no expression tree, so the default
        ``None`` is a HEURISTIC, not UFL's estimate (a product of two transcendental factors would be 6 there, a polynomial its own
        degree): it looks at the samples of the first, the middle and the last macro cell -- piecewise constant on every micro
        element, or only a handful of distinct values over the cell -> centroid rule (degree 0), anything else -> degree 3 --
        logs the choice with its evidence at WARNING level and raises when the three cells disagree.  Pass an integer to choose
        the rule yourself; ``TwoPhase`` / ``Separable`` coefficients carry their own degree and never guess, and an ``Expression`` has
        a tree: its degree is estimated from it by UFL's rules (``Expression.degree``), nothing is sampled and nothing is logged.
        ``device``: HIP device ordinal; resolved at the first solve (``dist.default_device``: the ordinal given to
        ``dist.select_device``, the process group's bound device, the torch device the caller selected, else LOCAL_RANK modulo the
        visible devices, else 0).
        ``reserve``: create the plan and allocate its device workspace for this rank's share of the macro cells NOW (``prepare()``)
        instead of inside the first ``solve()`` -- the nested-dissection route of the C4 / C5 size holds 0.2 GB of fronts per cell
        of a chunk, 0.5 - 3 s of ``hipMalloc`` that the first assembly would otherwise hide.  Resolves the device at construction
        time, so leave it off when the solver is built before ``init_process_group``; ``prepare()`` can be called later.
        ``tree_loads``: the plan is created with ``tree_loads=True`` (``MicroCellPlan``): where it takes a nested-dissection route, the
        load solves of ``load_response()``, ``criterion()``, ``solve_nonlinear(load=True)`` and the second derivatives substitute on
        the kept fronts instead of eliminating again.  Off by default; the sibling plan of ``method="newton"`` never needs it."""
        self._logger = logging.getLogger(__name__)
        self._msh = msh
        self._comm = msh.comm
        self._coeff = A
        self._f = f
        self._eps = eps
        self._cell_mesh = msh_micro
        self._tdim = msh.topology.dim
        if self._tdim not in (2, 3):
            raise ValueError("Topology should be 3D or 2D")  # hmm.py:104-105
        if self._tdim != msh.geometry.dim:
            raise ValueError(
                "Topological dimension is different from geometrical dimension. Currently surfaces in 3D are not supported."
            )
        if msh_micro.topology.dim != msh_micro.geometry.dim:
            raise ValueError("Topological dimension is different from geometrical dimension for micro mesh.")
        if self._tdim != msh_micro.topology.dim:
            raise ValueError("Micro and macro mesh should have the same dimensionality.")  # hmm.py:114-115
        try:
            self._n_micro = micro_cells_per_side(msh_micro)
        except ValueError:  # any other periodic unit-cell mesh: the mesh route (MicroCellPlan.from_mesh)
            self._n_micro = None
        self._cell_mesh_area = float(msh_micro.cell_volumes().sum())  # hmm.py:101
        if isinstance(A, TwoPhase) and quadrature_degree not in (None, 0, 1):
            raise ValueError("a TwoPhase coefficient is piecewise constant in y (UFL: degree 0, centroid rule); "
                             f"quadrature_degree={quadrature_degree} would be ignored by the device sampler")
        self._quadrature_degree = quadrature_degree  # None: decided from the samples on first use (quadrature_degree_used)
        self.quadrature_degree_used: int | None = 0 if isinstance(A, TwoPhase) else quadrature_degree
        if isinstance(A, (Separable, Expression)) and quadrature_degree is None:
            self.quadrature_degree_used = A.degree
        self._rhs_degree = rhs_quadrature_degree
        self._device = device  # None: resolved lazily in _ensure_plan (the solver may be built before init_process_group)
        self._reserve_at_construction = bool(reserve)
        self._plan_options = {"tree_loads": True} if tree_loads else {}  # what both kinds of plan are asked for beside the defaults

        self._V_macro = self._setup_macro_function_space()
        self._macro_coordinates = self._V_macro.tabulate_dof_coordinates()
        self._bs = self._V_macro.bs
        self._num_basis_functions_per_cell = (self._tdim + 1) * self._bs  # hmm.py:138-140
        self._num_global_dofs = self._V_macro.num_dofs
        self._u = fem.Function(self._V_macro)
        self._A = None
        self._needs_reassembly = True
        if petsc_options_cell_problem is None:
            petsc_options_cell_problem = {"ksp_atol": 1e-10}  # hmm.py:153-155 (advisory here)
        self._petsc_options_cell_problem = petsc_options_cell_problem
        self._petsc_options_global_solve = petsc_options_global_solve
        self._petsc_options_prefix = petsc_options_prefix
        self._bcs: list[fem.DirichletBC] = []
        self.secant: SecantResult | None = None  # solve_nonlinear: the last step's result per cell
        self.nonlinear_history: list[float] = []  # ... and the relative macro change of every step
        self.tangent_tensors = None  # D = d sigma_H / d xi per macro cell of the last solve_nonlinear(method="newton")
        self.history = None  # [cells of this rank, n_el, n_history]: the committed history variables of a law that has some
        self.history_trial = None  # ... and what the last step of the last solve_nonlinear left: commit_history() makes it the state
        self._nonlinear_state = None  # what defines the state the last solve_nonlinear ended in (criterion / reconstruct(nonlinear=True))
        self._linearisation_load = None  # P_T of the macro step solve() is serving (solve_nonlinear sets and clears it)
        self._nonlinear_load = False  # solve() serves a step of solve_nonlinear(load=True): the load is inside _linearisation_load
        self._tangent_plan = None  # the sibling plan of the tangent kind (solve_nonlinear(method="newton") builds and keeps it)
        self._tangent_reserved = 0  # ... and the cells it is reserved for
        self._Dtheta_t = None
        self._plan: MicroCellPlan | None = None
        self._reserved_cells = 0
        self.effective_tensors: np.ndarray | None = None  # A_H / C_H of every macro cell after assembly
        self.cell_info: np.ndarray | None = None
        self._solved = False  # reconstruct() defaults to the last solve() result
        self._polarisation = None  # set_polarisation / set_eigenstrain
        self._eigenstrain = False  # what _polarisation holds is an eigenstrain E: the load is -A : E
        self._polarisation_fields: np.ndarray | None = None  # set_polarisation_fields: [num_cells, n_fields] of a load Expression with fields
        self._fields: np.ndarray | None = None  # set_fields: [num_cells, n_fields] of an Expression with fields
        self.effective_polarisation: np.ndarray | None = None  # P_eff[N, t] of every macro cell after a solve() with a polarisation
        if self._reserve_at_construction:
            self.prepare()

    # -- API ---------------------------------------------------------------------------------------
    @property
    def function_space(self) -> fem.FunctionSpace:
        """Function space of the macro mesh (hmm.py:173-176)."""
        return self._V_macro

    def set_boundary_conditions(self, bcs):
        """hmm.py:276-287."""
        self._bcs = bcs if isinstance(bcs, list) else [bcs]
        self._needs_reassembly = True

    def set_right_hand_side(self, f: Callable):
        """hmm.py:289-296."""
        self._f = f

    def set_parameters(self, p):
        """New values of the parameters ``p[k]`` of an ``Expression`` coefficient (``Expression.with_parameters``: nothing is parsed
        again).  The macro matrix is reassembled by the next ``solve()``; the plan and its workspace are kept -- the step of a
        calibration loop.  ``ValueError`` when the coefficient is no ``Expression`` with parameters, or ``p`` has another length."""
        if not isinstance(self._coeff, Expression) or self._coeff.n_params == 0:
            raise ValueError("set_parameters() needs an Expression coefficient with parameters (Expression(..., p=[...]))")
        self._coeff = self._coeff.with_parameters(p)
        self._needs_reassembly = True

    def set_fields(self, values):
        """The values of the fields ``f[k]`` of an ``Expression`` coefficient (``Expression(..., fields=...)``), one per macro cell: a
        design variable, the macro solution at the midpoint (``cell_means``), a random draw.  ``values``: an array
        ``[num_cells, n_fields]`` (``[num_cells]`` is accepted for one field), or a callable ``x[3, num_cells] -> [n_fields, num_cells]``
        evaluated at the cell midpoints.  Every value must be finite.  The macro matrix is reassembled by the next ``solve()``; the
        plan and its workspace are kept -- the step of a Picard loop or of a design iteration.  Under a process group every rank is
        given the whole array and reads the rows of its own cells.  ``ValueError`` when the coefficient is no ``Expression`` with
        fields, or ``values`` has another shape."""
        co = self._coeff
        if not isinstance(co, Expression) or co.n_fields == 0:
            raise ValueError("set_fields() needs an Expression coefficient with fields (Expression(..., fields=...))")
        self._fields = self._field_values(co, values)
        self._needs_reassembly = True

    def _field_values(self, co: Expression, values) -> np.ndarray:
        """``values`` of the fields of the expression ``co`` as float64[num_cells, n_fields], every value finite (``set_fields``: the
        shapes it takes)."""
        n, k = self._msh.num_cells, co.n_fields
        if callable(values):
            v = np.asarray(values(self._msh.cell_midpoints().T), dtype=np.float64)
            v = (v[None] if v.ndim == 1 and k == 1 else v).T
        else:
            v = np.asarray(values, dtype=np.float64)
            if v.ndim == 1 and k == 1:
                v = v[:, None]
        if v.shape != (n, k):
            raise ValueError(f"the fields {', '.join(co.field_names)} need values of shape ({n}, {k}); got {np.shape(values) if not callable(values) else v.T.shape}")
        if not np.isfinite(v).all():
            c, j = np.argwhere(~np.isfinite(v))[0]
            raise ValueError(f"field {co.field_names[j]} is not finite on macro cell {c}: {v[c, j]}")
        return np.array(v, dtype=np.float64, order="C")

    def cell_means(self, u=None) -> np.ndarray:
        """[num_cells] (a scalar macro space) or [num_cells, d]: the mean of the vertex values of the macro field ``u`` (a macro
        ``fem.Function`` or its dof array; default: the last ``solve()`` result) on every macro cell -- u_H at the cell midpoint, what a
        solution-dependent coefficient ``A(x, u_H(x), y)`` is fed: ``h.set_fields(h.cell_means(u))``."""
        uT = self._macro_dofs(self._or_last_solve(u, "cell_means"))[self._cell_dofs()]  # [nc, (d + 1) * bs], dof = vertex * bs + component
        mean = uT.reshape(uT.shape[0], -1, self._bs).mean(axis=1)
        return mean[:, 0] if self._bs == 1 else mean

    # -- the arguments every method takes --------------------------------------------------------------
    def _or_last_solve(self, u, method: str):
        """``u`` of the public method ``method``: None means the last ``solve()`` result."""
        if u is None:
            if not self._solved:
                raise RuntimeError(f"{method}() needs a macro solution: call solve() first or pass u")
            u = self._u
        return u

    def _macro_dofs(self, u, subject: str = "u") -> np.ndarray:
        """The dof vector of a macro field (a macro ``fem.Function`` or its dof array), checked against the macro space."""
        x = np.asarray(u.x.array if hasattr(u, "x") else u, dtype=float)
        if x.shape != (self._num_global_dofs,):
            raise ValueError(f"{subject} has {x.size} dofs; the macro space has {self._num_global_dofs}")
        return x

    def _cells_argument(self, cells, method: str, local: bool) -> np.ndarray:
        """``cells`` of the public method ``method`` as int64[N], N >= 1: None means every macro cell, or (``local``) this rank's."""
        if cells is None:
            cells = self._local_cells() if local else np.arange(self._msh.num_cells)
        else:
            cells = np.asarray(cells, dtype=np.int64).ravel()
        if len(cells) == 0:
            raise ValueError(f"{method}() needs at least one macro cell")
        return cells

    def _cell_dofs(self, cells=slice(None)) -> np.ndarray:
        """[N, nb]: the macro dofs of ``cells`` (default: every macro cell), dof = vertex * bs + component."""
        return _unroll_dofs(self._msh.cells[cells].astype(np.int64), self._bs)

    def _volume_ratio(self, cells=slice(None)) -> np.ndarray:
        """vol(T) / vol(Y) of ``cells`` (default: every macro cell)."""
        return self._msh.cell_volumes()[cells] / self._cell_mesh_area

    def _cell_rows(self, cells: np.ndarray, coeff=None) -> np.ndarray:
        """x of ``coeff`` (default: the coefficient) on ``cells``: the midpoints [N, 3] and, for an ``Expression`` with fields, the fields
        of the cells after them, [N, 3 + n_fields] -- the rows the device reads and the x every host path evaluates the expression at."""
        c = self._msh.cell_midpoints()[cells]
        co = self._coeff if coeff is None else coeff
        if not isinstance(co, Expression) or co.n_fields == 0:
            return c
        if self._fields is None or self._fields.shape[1] != co.n_fields:
            raise RuntimeError(f"the Expression reads the fields {', '.join(co.field_names)}: call set_fields() with their values per macro cell first")
        return np.concatenate([c, self._fields[cells]], axis=1)

    def set_polarisation(self, P):
        """A prescribed micro flux / stress field P(x, y): a thermal eigenstress -A : alpha dT, a prestress, the gravity
        term of Darcy flow.  The micro total flux becomes A (grad / eps of the reconstruction) + P, and ``solve()`` adds the load
        b_T = -vol(T)/vol(Y) (macro strains of the basis functions) . P_eff[T] of the effective polarisation of every macro cell.

        ``P``: a NumPy-vectorised callable ``P(x, y) -> [t, ...]`` (components in the order of ``Reconstruction.flux``: the flux vector, or
        s00, s11[, s22], s01[, s02, s12], shear not doubled), sampled with the micro rule that samples the coefficient; an array
        ``[n_el, t]`` of element means shared by all macro cells; an array ``[N, n_el, t]``; ``None`` removes it (``solve()`` is then bit
        for bit what it is without this call).

        ``P`` may also be a vector ``Expression`` with t components (``Expression(["...", ...])``): it is sampled ON THE DEVICE, at the
        points that sample the coefficient -- only its program and one row per macro cell cross the boundary (hommx_loads_source,
        HOMMX_LOADS_PROGRAM).  Its parameters change through ``P.with_parameters(p)`` and this call again (the plan is kept), its
        fields ``f[k]`` are its own: ``set_polarisation_fields``.  A plan stand-in without the capability is given the element means
        of the expression, as of a callable.  Replaces an eigenstrain (``set_eigenstrain``)."""
        self._set_load(P, False)

    def set_eigenstrain(self, E):
        """A prescribed micro eigenstrain E(x, y): a thermal strain alpha dT, a swelling, a misfit.  The polarisation is the eigenstress
        ``P = -A : E``, formed ON THE DEVICE from the coefficient as it is sampled there (hommx_loads_source,
        HOMMX_LOADS_EIGENSTRAIN), whatever the form of the coefficient: nobody multiplies by the stiffness by hand.

        ``E`` takes what ``set_polarisation`` takes -- a callable ``E(x, y) -> [t, ...]``, ``[n_el, t]``, ``[N, n_el, t]``, a vector
        ``Expression`` with t components, ``None`` --, with the components in the order and convention of ``Reconstruction.strain``:
        Poisson a gradient; elasticity e00, e11[, e22], then the DOUBLED shears 2 e01[, 2 e02, 2 e12].  Replaces a polarisation.  A
        plan stand-in without the capability is given ``-material(element means of A) E`` formed on the host (``eigenstress``)."""
        self._set_load(E, True)

    def _set_load(self, P, eigenstrain: bool):
        what = "E" if eigenstrain else "P"
        t = self._tensor_size()
        if isinstance(P, Expression):
            if P.shape != "vector" or P.n_comp != t:
                raise ValueError(f"an Expression for {what} must be a vector of {t} components (Expression([c0, c1, ...])); got a {P.shape} "
                                 f"of {P.n_comp}")
            if P.n_y > self._tdim:
                raise ValueError(f"the Expression reads y[{P.n_y - 1}]; the micro mesh has {self._tdim} dimensions")
        elif P is not None and not callable(P):
            P = np.ascontiguousarray(P, dtype=float)
            n_el = self._cell_mesh.num_cells
            if P.shape not in ((n_el, t), (self._msh.num_cells, n_el, t)):
                raise ValueError(f"{what} has shape {P.shape}; expected ({n_el}, {t}) or ({self._msh.num_cells}, {n_el}, {t})")
        self._polarisation = P
        self._eigenstrain = bool(eigenstrain) and P is not None
        self.effective_polarisation = None

    def set_polarisation_fields(self, values):
        """The values of the fields ``f[k]`` of the LOAD expression (``set_polarisation`` / ``set_eigenstrain`` of an
        ``Expression(..., fields=...)``), one per macro cell -- the temperature change of a thermal strain, say: the shapes, the
        finiteness check and the process-group rule of ``set_fields``.  They are the load's own: the coefficient's fields are
        ``set_fields``.  The plan is kept.  ``ValueError`` when the load is no ``Expression`` with fields."""
        P = self._polarisation
        if not isinstance(P, Expression) or P.n_fields == 0:
            raise ValueError("set_polarisation_fields() needs a polarisation or an eigenstrain given as an Expression with fields "
                             "(Expression([...], fields=...))")
        self._polarisation_fields = self._field_values(P, values)
        self.effective_polarisation = None

    def _load_rows(self, cells: np.ndarray) -> np.ndarray:
        """The rows of the load expression on ``cells``: the midpoints [N, 3] and, for one with fields, its own fields after them."""
        c, P = self._msh.cell_midpoints()[cells], self._polarisation
        if P.n_fields == 0:
            return c
        if self._polarisation_fields is None or self._polarisation_fields.shape[1] != P.n_fields:
            raise RuntimeError(f"the load Expression reads the fields {', '.join(P.field_names)}: call set_polarisation_fields() with their "
                               "values per macro cell first")
        return np.concatenate([c, self._polarisation_fields[cells]], axis=1)

    @abstractmethod
    def _setup_macro_function_space(self) -> fem.FunctionSpace: ...

    # -- coefficient sampling (hmm.py:190-198, 349-352) ---------------------------------------------
    def _sample_one(self, c_T: np.ndarray, yq: np.ndarray, coeff=None):
        """A(c_T, y) at the quadrature points yq[dim, npts] -> array [npts, ...] (or Lame).  ``coeff``: another callable of the
        coefficient's shape (a direction of ``tensor_derivatives``) instead of A."""
        v = (coeff or self._coeff)(c_T, yq)
        if isinstance(v, Lame):
            return _lame_stacked(v, (yq.shape[1],))
        v = np.asarray(v, dtype=float)
        if v.ndim == 0 or v.shape[0] != yq.shape[1]:
            v = np.broadcast_to(v, (yq.shape[1],) + v.shape).copy()
        return v

    def _quadrature_points(self, degree: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """(yq[n_el, n_q, d], w[n_q]): points and weights of the micro rule of ``degree`` on every micro element.  Default: the degree
        that samples the coefficient (``quadrature_degree_used``, decided from the samples when nobody chose it)."""
        if degree is None:
            if self.quadrature_degree_used is None:
                self.quadrature_degree_used = self._auto_quadrature_degree()
            degree = self.quadrature_degree_used
        bary, w = micro_quadrature(self._tdim, degree)
        return np.einsum("qa,eak->eqk", bary, self._cell_mesh.cell_vertices()), w

    def _quadrature_evidence(self, c_T: np.ndarray) -> tuple[int, str]:
        """Degree the heuristic picks from the samples of ONE macro cell, and why."""
        d = self._tdim
        yq, _ = self._quadrature_points(3)
        v = self._sample_one(c_T, yq.reshape(-1, d).T)
        v = v.reshape((yq.shape[0], yq.shape[1]) + v.shape[1:])
        if np.all(v == v[:, :1]):
            return 0, "constant on every micro element"
        flat = v.reshape(v.shape[0] * v.shape[1], -1)
        distinct = max(int(np.unique(flat[:, k]).size) for k in range(flat.shape[1]))
        if distinct <= 8:
            return 0, f"{distinct} distinct values over the cell (a conditional whose interface cuts elements)"
        return 3, f"{distinct} distinct values over the cell, varying inside elements (smooth in y)"

    def _auto_quadrature_degree(self, c_T: np.ndarray | None = None) -> int:
        """Default policy (see __init__): sample A(c_T, .) at the degree-3 points of every micro element of the first, the middle
        and the last macro cell.  A ``conditional`` between constants (UFL: degree 0, centroid rule) shows up as a coefficient
        that is constant on every element or -- when its interface cuts through elements, like the wrapped disc of
        inclusion.py:107-118 -- takes only a handful of distinct values over the whole cell; anything else is treated as smooth:
        degree 3.  The choice is logged with its evidence; cells that disagree raise (a wrong guess would silently solve a
        different discrete problem from the reference's)."""
        mid = self._msh.cell_midpoints()
        probe = [0, len(mid) // 2, len(mid) - 1] if c_T is None else [None]
        found = [self._quadrature_evidence(mid[k] if k is not None else c_T) for k in probe]
        degrees = sorted({f[0] for f in found})
        if len(degrees) > 1:
            raise ValueError("cannot guess the micro quadrature degree of A(x, y): macro cells " + ", ".join(
                f"{k}: degree {f[0]} ({f[1]})" for k, f in zip(probe, found)) + " -- pass quadrature_degree= explicitly "
                "(0 for a conditional between constants, 3 for one transcendental function of y: what UFL estimates, hmm.py:190-198)")
        self._logger.warning("quadrature_degree not given: guessed degree %d for A(x, y) from its samples (%s); pass "
                             "quadrature_degree= to choose the rule UFL would estimate for your expression",
                             degrees[0], "; ".join(f"cell {k}: {f[1]}" for k, f in zip(probe, found)))
        return degrees[0]

    def _element_means(self, cells: np.ndarray, coeff=None) -> tuple[np.ndarray, str]:
        return self._pack_coefficient(self._sampled_means(cells, coeff))

    def _sampled_means(self, cells: np.ndarray, coeff=None, rows: np.ndarray | None = None) -> np.ndarray:
        """Element means [N, n_el, ...] of ``coeff`` (default: the coefficient) on the sampling boxes of ``cells``, as sampled.
        ``rows``: the x of ``coeff`` on ``cells`` when it is not that of the coefficient (``_load_rows``)."""
        yq, w = self._quadrature_points()
        n_el, nq = yq.shape[:2]
        yflat = yq.reshape(-1, self._tdim).T
        c = self._cell_rows(cells, coeff) if rows is None else rows
        out = self._sample_batched(c, yflat, n_el, nq, w, coeff)
        if out is None:  # the callable is not broadcastable over cells: one call per macro cell (as the reference)
            first = self._sample_one(c[0], yflat, coeff)
            out = np.empty((len(cells),) + (n_el,) + first.shape[1:])
            for k in range(len(cells)):
                v = first if k == 0 else self._sample_one(c[k], yflat, coeff)
                out[k] = np.tensordot(w, v.reshape((n_el, nq) + v.shape[1:]), axes=([0], [1]))
        return out

    def _sample_batched(self, c: np.ndarray, yflat: np.ndarray, n_el: int, nq: int, w: np.ndarray, coeff=None):
        """Try ONE broadcast call A(x[3, N_c, 1], y[d, 1, npts]) -> [N_c, npts(, ...)] per chunk of cells; accept it only
        if it reproduces the per-cell call on the first and last cell.  Returns None when the callable cannot broadcast."""
        nc, npts = c.shape[0], yflat.shape[1]
        if nc < 4:
            return None
        try:
            ref0 = self._sample_one(c[0], yflat, coeff)
            ref1 = self._sample_one(c[-1], yflat, coeff)
            chunk = max(1, int(2.0e7 // max(1, npts)))
            parts = []
            for a in range(0, nc, chunk):
                xb = c[a : a + chunk].T[:, :, None]
                v = (coeff or self._coeff)(xb, yflat[:, None, :])
                if isinstance(v, Lame):
                    v = _lame_stacked(v, (xb.shape[1], npts))
                else:
                    v = np.asarray(v, dtype=float)
                    if v.ndim < 2 or v.shape[:2] != (xb.shape[1], npts):
                        if v.ndim >= 2 and v.shape[:2] == (1, npts) or v.ndim == 0:
                            v = np.broadcast_to(v, (xb.shape[1], npts) + v.shape[2:]) if v.ndim else np.full((xb.shape[1], npts), float(v))
                        else:
                            return None
                if nq == 1:  # centroid rule: the mean IS the sample (no copy)
                    parts.append(v.reshape((v.shape[0], n_el) + v.shape[2:]))
                else:
                    parts.append(np.tensordot(v.reshape((v.shape[0], n_el, nq) + v.shape[2:]), w, axes=([2], [0])))
            out = parts[0] if len(parts) == 1 else np.concatenate(parts, axis=0)
            chk0 = np.tensordot(w, ref0.reshape((n_el, nq) + ref0.shape[1:]), axes=([0], [1]))
            chk1 = np.tensordot(w, ref1.reshape((n_el, nq) + ref1.shape[1:]), axes=([0], [1]))
            if out[0].shape != chk0.shape or not (np.allclose(out[0], chk0, rtol=1e-14, atol=0) and np.allclose(out[-1], chk1, rtol=1e-14, atol=0)):
                return None
            return out
        except Exception:
            return None

    def _pack_coefficient(self, means: np.ndarray) -> tuple[np.ndarray, str]:
        """Element means -> the layout of include/hommx_hip.h for the plan kind."""
        d = self._tdim
        if self._kind == "poisson":
            if means.ndim == 2:
                return means, "poisson"
            if means.shape[-2:] == (d, d):
                asym = np.abs(means - np.swapaxes(means, -1, -2)).max() if means.size else 0.0
                if asym > 1e-12 * max(1.0, float(np.abs(means).max())):
                    raise ValueError("matrix-valued A must be symmetric: the kernels form the Schur complement C0 - B^T K^+ B, which "
                                     "equals the reference's energy functional (hmm.py:652-667) only for symmetric A "
                                     f"(max |A - A^T| = {asym:.3e})")
                pairs = _VOIGT[d]
                return np.stack([0.5 * (means[..., i, j] + means[..., j, i]) for i, j in pairs], axis=-1), "poisson_matrix"
            raise ValueError(f"PoissonHMM coefficient must be scalar or {d}x{d}; got trailing shape {means.shape[2:]}")
        if means.ndim == 3 and means.shape[-1] == 2:
            return means, "elasticity"
        if means.shape[-4:] == (d, d, d, d):
            cv = hooke_to_voigt(means, d)
            t = cv.shape[-1]
            iu = np.triu_indices(t)
            return cv[..., iu[0], iu[1]], "elasticity_voigt"
        raise ValueError("elasticity coefficient must be Lame(lam, mu) or a [d,d,d,d] tensor")

    def _stratification(self, cells: np.ndarray) -> np.ndarray | None:
        """M[c] = Dtheta_transpose(c_T) of the given macro cells (hmm.py:756-757, 1015-1016).  ONE broadcast call
        ``Dtheta_transpose(x[3, N_c]) -> [d, d, N_c]`` when the callable allows it (accepted only if it reproduces the per-cell
        call on the first and the last cell), else one call per cell as the reference does."""
        if self._Dtheta_t is None:
            return None
        return self._matrix_at_midpoints(self._Dtheta_t, cells, "Dtheta_transpose")

    def _matrix_at_midpoints(self, fn, cells: np.ndarray, name: str) -> np.ndarray:
        """[N_c, d, d]: the matrix-valued callable ``fn`` (``Dtheta_transpose`` or its derivative with respect to a design parameter) at
        the midpoints of the given macro cells, by the rule of ``_stratification``."""
        c = self._msh.cell_midpoints()[cells]
        d = self._tdim
        nc = len(cells)

        def one(x):
            m = np.asarray(fn(x), dtype=float)
            if m.shape != (d, d):
                raise ValueError(f"{name} must return a {d}x{d} matrix (hmm.py:741, :762); got {m.shape}")
            return m

        if nc == 0:
            return np.empty((0, d, d))
        first, last = one(c[0]), one(c[-1])
        known = {0: first, nc - 1: last}
        if nc >= 4:
            # the broadcast result is accepted only if it reproduces the per-cell call (what the reference does, hmm.py:756-757) on the
            # first, the middle, the last and a few more cells spread over the batch -- a callable that broadcasts but reduces over its
            # argument, or indexes into it, agrees at the ends at best
            probe = sorted({nc // 2, nc // 3, (2 * nc) // 3, (7 * nc) // 11, 1, nc - 2} - {0, nc - 1})
            try:
                rows = fn(c.T)
                mb = np.empty((d, d, nc))
                for i in range(d):
                    for j in range(d):
                        mb[i, j] = np.broadcast_to(np.asarray(rows[i][j], dtype=float), (nc,))
                mb = np.ascontiguousarray(np.moveaxis(mb, -1, 0))
                for k in probe:
                    known[k] = one(c[k])
                if all(np.array_equal(mb[k], v) for k, v in known.items()):
                    return mb
                self._logger.debug(f"{name}: the broadcast call disagrees with the per-cell calls; evaluating cell by cell")
            except Exception as exc:
                self._logger.debug(f"{name}: no broadcast evaluation ({type(exc).__name__}: {exc}); evaluating cell by cell")
        M = np.empty((nc, d, d))
        for k in range(nc):
            M[k] = known[k] if k in known else one(c[k])
        return M

    # -- the hot path (replaces the loop hmm.py:298-332) ---------------------------------------------
    @staticmethod
    def _sharded() -> bool:
        """Only shard when the caller already runs under an initialised torch.distributed group with more than one rank."""
        import sys

        dist = sys.modules.get("torch.distributed")
        return dist is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def _ensure_plan(self, kind: str, n_cells: int | None = None) -> MicroCellPlan:
        """The plan of this solver (created on first use: replaces the per-solve object construction of hmm.py:420-425).  With
        ``n_cells`` (``prepare()`` / ``reserve=True``) the plan's device workspace is allocated for batches of that size right away
        (``hommx_plan_reserve``); a solve without it allocates what its first batch needs (half as much on the C4 / C5 route: a caller
        who pays ahead of many batches gets the bigger chunks, one who pays inside the only solve does not want to)."""
        if self._plan is None or self._plan.kind != kind:
            if self._device is None:
                from .dist import default_device

                self._device = default_device()
            if self._n_micro is None:
                # load_solve: the frontal route serves load_response() and the second derivatives as every other route does
                self._plan = MicroCellPlan.from_mesh(self._cell_mesh, kind, device=self._device, load_solve=True, **self._plan_options)
            else:
                self._plan = MicroCellPlan(self._tdim, self._n_micro, kind, device=self._device, **self._plan_options)
            self._reserved_cells = 0
        if n_cells and n_cells > self._reserved_cells:
            self._plan.reserve(int(n_cells))
            self._reserved_cells = int(n_cells)
            if self._tangent_plan is not None:  # the sibling of solve_nonlinear(method="newton") follows every reservation
                self._ensure_tangent_plan(self._plan)
        return self._plan

    def _local_cells(self) -> np.ndarray:
        """The macro cells this rank solves (``_local_cell_count``): all of them, or its block under a process group."""
        n = self._msh.num_cells
        if self._sharded():
            import torch.distributed as dist

            from .dist import shard_range

            b, e, _ = shard_range(n, dist.get_rank(), dist.get_world_size())
            return np.arange(b, e)
        return np.arange(n)

    def _local_cell_count(self) -> int:
        """Macro cells this rank solves (hmm.py:307-310)."""
        return len(self._local_cells())

    def prepare(self, newton: bool = False) -> "BaseHMM":
        """Create the plan and allocate its device workspace for this rank's share of the macro cells now, so that the first
        ``solve()`` does not pay for it (not in the reference's API: there every PETSc object is made per solve, hmm.py:420-425).
        The kernel family depends on the coefficient's shape, which a plain callable only shows when sampled: one macro cell is
        sampled for that.  ``newton``: the sibling plan of ``solve_nonlinear(method="newton")`` as well; once that plan exists
        (built here or by the first Newton step) it is reserved with the plan, by this call and by ``reserve=True`` alike."""
        kind = self._micro_kind() if self._device_form() else self._element_means(np.array([0]))[1]
        plan = self._ensure_plan(kind, self._local_cell_count())
        if newton or self._tangent_plan is not None:
            self._ensure_tangent_plan(plan)
        return self

    def _shard_device(self):
        """Device of the gather buffer under RCCL = the plan's device (None before a plan exists on a gloo / stub-plan run)."""
        return self._plan.device if isinstance(self._plan, MicroCellPlan) else self._device

    def _tensor_size(self) -> int:
        d = self._tdim
        return d if self._kind == "poisson" else d * (d + 1) // 2

    def _micro_kind(self) -> str:
        """Plan kind of the coefficient forms that are sampled on the device (scalar / Lame values; the matrix of an ``Expression``)."""
        if self._kind == "poisson":
            return "poisson_matrix" if isinstance(self._coeff, Expression) and self._coeff.shape == "matrix" else "poisson"
        return "elasticity"

    def _device_form(self) -> str | None:
        """Plan method that samples this coefficient on the device, or None for sampled element means."""
        co = self._coeff
        if isinstance(co, TwoPhase):
            return "solve_two_phase"
        if isinstance(co, Separable) and (self._kind == "poisson" or co.family == "affine"):  # Lame-valued: affine only
            return "solve_separable"
        if isinstance(co, Expression):
            fits = ("scalar", "matrix") if self._kind == "poisson" else ("lame",)
            if co.shape not in fits or (co.shape == "matrix" and co.dim != self._tdim):
                raise ValueError(f"an Expression for {type(self).__name__} must be " + (
                    f"a scalar or a symmetric {self._tdim} x {self._tdim} matrix" if self._kind == "poisson" else "Expression(lam=..., mu=...)")
                    + f"; got a {co.shape}" + (f" of size {co.dim}" if co.shape == "matrix" else ""))
            if co.n_y > self._tdim:
                raise ValueError(f"the Expression reads y[{co.n_y - 1}]; the micro mesh has {self._tdim} dimensions")
            return "solve_program"
        return None

    def _sampled_on_device(self) -> str | None:
        """The plan method that samples this coefficient on the device WITH THE PLAN THAT STANDS HERE, or None for sampled element
        means: the coefficient has a device form (``_device_form``) and the plan offers that method -- a ``MicroCellPlan`` offers all
        of them, a stand-in may not (``_coef_stream``).  This is the one place that asks."""
        form = self._device_form()
        return form if form is not None and hasattr(self._ensure_plan(self._micro_kind()), form) else None

    def _coef_stream(self, cells: np.ndarray) -> tuple[CoefStream, str]:
        """The coefficient of ``cells`` as the plan takes it, and the plan kind: ``TwoPhase`` as one mask (evaluated at the element
        barycentres) + two values per cell, ``Separable`` as one table of g + (a, b) per cell (per Lame parameter for the elasticity
        classes: test_integration_linear_elasticity.py:78-93), an ``Expression`` as its program + the points of the micro quadrature rule
        + the midpoint (and the fields, ``set_fields``) of every cell, anything else as sampled element means.

        What stands in ``self._plan`` is a ``MicroCellPlan`` or a stand-in for it (the CPU tests answer from a NumPy restatement).  A stand-in has
        ``t``, ``kind`` and ``solve(coef, M=None, return_info=False[, return_correctors])``; it may have ``reserve`` (needed by
        ``prepare()``), ``reconstruct``, ``device``, ``solve_two_phase``, ``solve_separable`` and ``solve_program``.  Without the last three it gets those
        coefficients as element means (``_sampled_on_device``: the one place that asks).  ``reconstruct(coef, xi, M, fields=...)`` is given element means
        as an array and a device-sampled coefficient as the ``CoefStream``, under the same rule.  ``loads(coef, P, M, per_cell=...,
        response=..., fields=..., return_correctors=...)`` is given the load as per-cell element means unless the stand-in says
        ``load_sources = True``: then an ``Expression`` load comes as its program ``CoefStream`` and an eigenstrain with
        ``eigenstrain=True`` (``_loads_on_device``: the one place that asks that)."""
        form = self._sampled_on_device()
        if form is None:
            coef, kind = self._element_means(cells)
            return CoefStream.sampled(coef), kind
        kind, co, c = self._micro_kind(), self._coeff, self._cell_rows(cells)
        if form == "solve_two_phase":
            mask = self._phase_mask()
            values = co.phase_values(c)
            if (values.ndim == 2) != (kind == "poisson"):
                raise ValueError("TwoPhase values must be scalars for PoissonHMM and Lame(lam, mu) for LinearElasticityHMM")
            return CoefStream.two_phase(mask, values), kind
        yq, w = self._quadrature_points()
        if form == "solve_program":
            return CoefStream.program(yq, w, *co.program(), co.n_comp, c, n_params=co.n_params, n_fields=co.n_fields), kind
        return CoefStream.separable(co.family, co.table(yq, w), w, co.params(c)), kind

    def _phase_mask(self) -> np.ndarray:
        """The indicator of a ``TwoPhase`` coefficient at the micro element barycentres."""
        return np.asarray(self._coeff.indicator(self._cell_mesh.cell_midpoints()[:, : self._tdim].T), dtype=bool)

    def _effective_tensors(self, cells: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """A_H / C_H and the per-cell info flags of ``cells``.  Under a process group every rank samples, uploads and solves
        ONLY its block of the cells (the reference's MPI partition, hmm.py:307-310); one all-gather returns the whole field and
        the real info vector to every rank (hommx_amd/dist.py)."""

        def block(b, e):
            stream, kind = self._coef_stream(cells[b:e])
            return self._ensure_plan(kind), stream, self._stratification(cells[b:e])

        if self._sharded():
            from .dist import run_sharded, solve_block

            return run_sharded(self._tensor_size(), len(cells), lambda b, e: solve_block(*block(b, e)), device=self._shard_device())
        plan, stream, M = block(0, len(cells))
        return stream.solve(plan, M, return_info=True)

    def _loads_on_device(self, kind: str) -> bool:
        """Whether THE PLAN THAT STANDS HERE takes a load as a program ``CoefStream`` and forms the eigenstress itself
        (``loads(..., eigenstrain=True)``): a ``MicroCellPlan`` says so with ``load_sources``; a stand-in without it gets per-cell
        element means of the polarisation, as ever (``_coef_stream``).  The one place that asks."""
        return bool(getattr(self._ensure_plan(kind), "load_sources", False))

    def _polarisation_loads(self, cells: np.ndarray, kind: str | None = None) -> tuple:
        """The load of ``cells`` as ``plan.loads`` takes it, one load: (P, per_cell, eigenstrain) with P[1, n_el, t] and per_cell False
        when every cell shares it, else P[N, 1, n_el, t] and True.  A callable is sampled where the coefficient is sampled
        (``_sampled_means``).  On a plan of kind ``kind`` that takes load sources (``_loads_on_device``) an ``Expression`` is its program
        ``CoefStream`` on the same points (per_cell None) and an eigenstrain crosses as it is, ``eigenstrain`` True; on every other plan
        the ``Expression`` is sampled like a callable and the eigenstress is formed here, from the element means of the coefficient."""
        device = kind is not None and self._loads_on_device(kind)
        P = self._load_input(cells, device)
        if not self._eigenstrain or device:
            return P + (self._eigenstrain,)
        coef, packed = self._element_means(cells)
        return np.ascontiguousarray(eigenstress(coef[:, None], packed, self._tdim, P[0])), True, False

    def _load_input(self, cells: np.ndarray, device: bool) -> tuple:
        """(P, per_cell) of ``_polarisation_loads``: what was set -- a polarisation or an eigenstrain -- on ``cells``."""
        P = self._polarisation
        if isinstance(P, Expression) and device:
            yq, w = self._quadrature_points()
            return CoefStream.program(yq, w, *P.program(), P.n_comp, self._load_rows(cells), n_params=P.n_params, n_fields=P.n_fields), None
        if not callable(P):
            return (P[None], False) if P.ndim == 2 else (P[cells][:, None], True)
        t = self._tensor_size()
        rows = self._load_rows(cells) if isinstance(P, Expression) else None

        def components_last(x, y):  # [t, ...] -> [..., t] over the broadcast of x and y: the layout the sampling takes a coefficient in
            v = P(x, y)
            if len(v) != t:
                raise ValueError(f"the polarisation P(x, y) must return {t} components; got {len(v)}")
            shape = np.broadcast(x[0], y[0]).shape
            return np.stack([np.broadcast_to(np.asarray(c, dtype=float), shape) for c in v], axis=-1)

        return np.ascontiguousarray(self._sampled_means(cells, components_last, rows)[:, None]), True

    def _plan_inputs(self, cells: np.ndarray, sample=None) -> tuple:
        """(plan, coef, M, sampled) of ``cells`` for the derived outputs of a plan (``reconstruct``, ``loads``, the sensitivities): the
        coefficient crosses the boundary as ``solve()`` sends it (``_coef_stream``).  ``sample(cells, kind)``: what else the caller
        samples on these cells (a polarisation, directions) -- after the coefficient and before the plan is asked for, so that what it
        raises comes first."""
        stream, kind = self._coef_stream(cells)
        coef = stream.per_cell if stream.method == "solve" else stream  # element means as the array every plan (and stand-in) takes
        sampled = None if sample is None else sample(cells, kind)
        return self._ensure_plan(kind), coef, self._stratification(cells), sampled

    def _chunks(self, cells: np.ndarray, chunk_cells: int | None, bytes_per_cell, call, sample=None) -> list:
        """The results of ``call(plan, coef, M, sampled, sub, b)`` on ``cells`` in chunks ``sub = cells[b:b + chunk_cells]`` with the
        ``_plan_inputs`` of each.  ``chunk_cells`` None: 256 MB of what ``bytes_per_cell()`` counts for one cell -- every method has its
        own figure, for what it streams."""
        ch = max(1, int((256 << 20) // bytes_per_cell() if chunk_cells is None else chunk_cells))
        return [call(*self._plan_inputs(cells[b:b + ch], sample), cells[b:b + ch], b) for b in range(0, len(cells), ch)]

    def _load_blocks(self, cells: np.ndarray, chunk_cells: int | None, bytes_per_cell=None, **kw) -> list:
        """``plan.loads`` of the polarisation on ``cells``, chunk by chunk."""
        def call(plan, coef, M, P, sub, b):
            return plan.loads(coef, P[0], M, per_cell=P[1], **(dict(eigenstrain=True) if P[2] else {}), **kw)

        return self._chunks(cells, chunk_cells, bytes_per_cell, call, lambda sub, kind: self._polarisation_loads(sub, kind))

    def _effective_polarisation(self, cells: np.ndarray) -> np.ndarray:
        """P_eff[N, t] of ``cells`` (Levin: from the canonical correctors, on every route).  Under a process group every rank solves its
        block and one more all-gather of t numbers per cell returns the field to every rank; a failing rank makes all ranks raise."""

        def block(b, e):
            (r,) = self._load_blocks(cells[b:e], e - b)
            return r.P_eff[:, 0], r.info

        if self._sharded():
            from .dist import run_sharded

            return run_sharded(self._tensor_size(), len(cells), block, device=self._shard_device(), shape=(self._tensor_size(),))[0]
        return block(0, len(cells))[0]

    def _strain_basis(self, cells: np.ndarray) -> tuple[np.ndarray, np.ndarray | None]:
        """G[c, a, i] = d phi_a / d x_i of the macro basis functions on ``cells`` and, for vector-valued spaces, W[c, b, m]: the Voigt
        strain (doubled shear) of the b-th basis function, b = a * bs + component.  For a scalar space the basis of xi is G itself (W None)."""
        d, bs = self._tdim, self._bs
        X = self._msh.cell_vertices()[cells]  # [nc, d+1, d]
        Minv = np.linalg.inv(np.concatenate([np.ones(X.shape[:2] + (1,)), X], axis=2))
        G = np.transpose(Minv[:, 1:, :], (0, 2, 1))
        if bs == 1:
            return G, None
        I = np.eye(d)
        eps = 0.5 * (np.einsum("pi,caj->capij", I, G) + np.einsum("pj,cai->capij", I, G))
        eps = eps.reshape(len(cells), (d + 1) * bs, d, d)
        return G, np.stack([eps[:, :, k, l] * (1.0 if k == l else 2.0) for (k, l) in _VOIGT[d]], axis=-1)

    def _local_stiffness_from_tensors(self, cells: np.ndarray, AH: np.ndarray) -> np.ndarray:
        """S_loc = vol(T)/vol(Y) * (macro gradients) A_H (macro gradients)^T  == hmm.py:361-369."""
        G, Wv = self._strain_basis(cells)
        vol = self._volume_ratio(cells)
        if Wv is None:
            return vol[:, None, None] * np.einsum("cai,cij,cbj->cab", G, AH, G)
        return vol[:, None, None] * np.einsum("cam,cmn,cbn->cab", Wv, AH, Wv)

    def _compute_local_stiffness(self, cell_index: int) -> np.ndarray:
        """Single-cell form of the reference seam (hmm.py:334-369): a batch of one."""
        cells = np.array([cell_index])
        AH, info = self._effective_tensors(cells)
        return self._local_stiffness_from_tensors(cells, AH)[0]

    def _periodic_to_micro_nodes(self) -> np.ndarray:
        """Micro-mesh node -> periodic unknown (the slave -> master map of cell_problem.py:38-300 on the torus)."""
        if self._n_micro is None:
            if self._plan is not None and self._plan.to_periodic is not None:
                return self._plan.to_periodic
            from .cell_problem import create_periodic_boundary_conditions

            return create_periodic_boundary_conditions(fem.FunctionSpace(self._cell_mesh, 1)).to_periodic
        n, d = self._n_micro, self._tdim
        g = np.rint(self._cell_mesh.geometry.x[:, :d] * n).astype(np.int64) % n
        return g @ (n ** np.arange(d))

    def correctors_for_cell(self, cell_index: int) -> list[fem.Function]:
        """The nb correctors of one macro cell as functions on the micro mesh -- what the reference leaves in
        ``self._correctors`` after ``_compute_local_stiffness(cell_index)`` (hmm.py:204-207, 354-358, 431).

        Computed from the canonical correctors chi_m returned by the GPU: the macro basis functions are affine on the
        sampling box, so corrector_i = eps * sum_m w_m(grad phi_i) chi_m, up to the additive constant
        the reference's Krylov solve leaves undetermined (returned mean-free)."""
        cells = np.array([cell_index])
        coef, kind = self._element_means(cells)
        M = self._stratification(cells)
        _, chi = self._ensure_plan(kind).solve(coef, M, return_correctors=True)  # [1, t, n^d * bs]
        G, W = self._strain_basis(cells)
        Wv = (G if W is None else W)[0]  # [nb, t]
        return self._on_micro_mesh(self._eps * (Wv @ chi[0]))  # [nb, n^d * bs]

    def _on_micro_mesh(self, rows: np.ndarray) -> list[fem.Function]:
        """rows[k, n_nodes * bs] on the periodic unknowns -> one function on the micro mesh per row."""
        idx = self._periodic_to_micro_nodes()
        V_micro = fem.FunctionSpace(self._cell_mesh, self._bs)
        out = []
        for row in rows:
            f = fem.Function(V_micro)
            f.x.array[:] = row.reshape(-1, self._bs)[idx].ravel()
            out.append(f)
        return out

    def _assemble_stiffness(self):
        """hmm.py:298-332 with the cell loop replaced by one batched call."""
        if not self._needs_reassembly:
            return
        cells = np.arange(self._msh.num_cells)
        AH, info = self._effective_tensors(cells)
        S = self._local_stiffness_from_tensors(cells, AH)
        bad = np.nonzero((info != 0) | np.isnan(S).any(axis=(1, 2)))[0]
        for c in bad:  # hmm.py:320-323: log, do not raise
            self._logger.error(f"Something went wrong when calculating local matrix on cell {c}")
        self._set_macro_matrix(S)
        self.effective_tensors, self.cell_info = AH, info

    def _set_macro_matrix(self, S: np.ndarray):
        """Local stiffness matrices S[nc, nb, nb] of all macro cells -> the CSR macro matrix (MatSetValues(ADD), hmm.py:325-330)."""
        dofs = self._cell_dofs()  # [nc, nb]
        nb = dofs.shape[1]
        rows = np.repeat(dofs, nb, axis=1).ravel()
        cols = np.tile(dofs, (1, nb)).ravel()
        N = self._num_global_dofs
        self._A = sp.coo_matrix((S.ravel(), (rows, cols)), shape=(N, N)).tocsr()
        self._needs_reassembly = False

    def _add_cell_load(self, b: np.ndarray, P: np.ndarray):
        """b += b_T = -vol(T)/vol(Y) (macro strains of the basis functions) . P[T] for a constant flux / stress P[N, t] per macro cell:
        how the effective polarisation and the constant part of a linearised response enter the macro load."""
        G, Wv = self._strain_basis(np.arange(self._msh.num_cells))
        bT = -self._volume_ratio()[:, None] * np.einsum("cbm,cm->cb", G if Wv is None else Wv, P)
        np.add.at(b, self._cell_dofs().ravel(), bT.ravel())

    def solve(self) -> fem.Function:
        """Assemble the LHS, RHS and solve the problem (hmm.py:434-491)."""
        self._assemble_stiffness()
        A = self._A.copy()
        b = fem.assemble_load_vector(self._V_macro, self._f, self._rhs_degree)
        if self._polarisation is not None and not self._nonlinear_load:  # b_T of the effective polarisation, before the Dirichlet lifting
            self.effective_polarisation = self._effective_polarisation(np.arange(self._msh.num_cells))
            self._add_cell_load(b, self.effective_polarisation)
        if self._linearisation_load is not None:  # ... and of a macro step of solve_nonlinear: P_T = sigma_T - D_T xi_T
            self._add_cell_load(b, self._linearisation_load)
        for bc in self._bcs:  # hmm.py:453-480, bc by bc
            idx, val = bc.unrolled()
            u_bc = np.zeros(self._num_global_dofs)
            u_bc[idx] = val
            b_lift = A @ u_bc
            b[idx] = val
            b -= b_lift
            A = _zero_rows_columns(A, idx)
            b[idx] = val
        # the reference caches the BC-modified matrix; keep the clean one and re-apply -- same result
        if np.isnan(b).any() or np.isnan(A.data).any():
            self._logger.error("Something went wrong in the global problem solve. NaN in the assembled system")
        x = spla.spsolve(A.tocsc(), b)
        self._u.x.array[:] = x
        self._solved = True
        return self._u

    def _macro_strains(self, cells: np.ndarray, u: np.ndarray) -> np.ndarray:
        """xi[c] of the macro field u on every cell: grad u_H|_T (Poisson), or the Voigt vector of eps(u_H)|_T with doubled shear -- W^T u_T
        with the W of ``_local_stiffness_from_tensors``, so that u_T . S_loc u_T = vol(T) xi . A_H xi."""
        G, Wv = self._strain_basis(cells)
        uT = u[self._cell_dofs(cells)]  # [nc, nb]
        if Wv is None:
            return np.einsum("ca,cai->ci", uT, G)
        return np.einsum("cb,cbm->cm", uT, Wv)

    def _region_labels(self, regions) -> tuple[np.ndarray, int] | None:
        """``regions`` of ``reconstruct`` as (labels[n_el] uint8, number of regions): ``True`` is the indicator of a ``TwoPhase``
        coefficient (region 0 outside, region 1 inside), a callable y[dim, n_el] -> int[n_el] is evaluated at the micro element midpoints
        -- both exactly where ``_coef_stream`` evaluates the indicator --, anything else is the labels themselves."""
        if regions is None:
            return None
        mid = self._cell_mesh.cell_midpoints()[:, : self._tdim].T
        if regions is True:
            if not isinstance(self._coeff, TwoPhase):
                raise ValueError("regions=True uses the indicator of a TwoPhase coefficient; pass labels or a callable for any other coefficient")
            return region_labels(np.asarray(self._coeff.indicator(mid), dtype=bool), mid.shape[1], 2)
        return region_labels(regions(mid) if callable(regions) else regions, mid.shape[1])

    def _secant_chunks(self, cells: np.ndarray, xi: np.ndarray, law: SecantLaw, rows: np.ndarray, points: np.ndarray, chunk_cells,
                       history: np.ndarray | None, load: bool, extra: int, kw, tangent: bool = False) -> SecantResult:
        """``plan.secant`` of ``law`` on ``cells``, chunk by chunk -> the joined ``SecantResult`` with ``cells``; ``tangent``:
        ``plan.secant_tangent`` on the sibling plan instead.  ``xi``, ``rows`` and ``history`` (None: a law without history variables)
        lie along ``cells`` and are sliced per chunk; ``kw(b, n)``: the other keyword arguments of the n cells from position b.
        ``load``: the solver's polarisation or eigenstrain, sampled chunk by chunk.  A chunk streams the iteration's own outputs, a
        sampled load, the history in and out, a sampled coefficient, and ``extra`` bytes per cell for what the caller adds."""
        t, n_el = self._tensor_size(), self._cell_mesh.num_cells

        def bytes_per_cell():
            out = 8 * (3 + t * t + t) + 4 + extra
            if load and not isinstance(self._polarisation, Expression):
                out += 8 * n_el * t  # a sampled load
            if history is not None:  # in and out
                out += 16 * n_el * history.shape[2]
            return out if self._sampled_on_device() else out + n_el * (1 if self._kind == "poisson" else 2) * 8

        def sample(sub, kind):  # (P, per_cell, eigenstrain) as plan.secant takes them
            return self._load_input(sub, self._loads_on_device(kind)) + (self._eigenstrain,)

        def call(plan, coef, M, P, sub, b):
            at = slice(b, b + len(sub))
            args = dict(rows=rows[at], points=points, **kw(b, len(sub)))
            if P is not None:
                args.update(P=P[0], per_cell=P[1], eigenstrain=P[2])
            if history is not None:
                args["history"] = history[at]
            if not tangent:
                return plan.secant(coef, xi[at], law, M, **args)
            return plan.secant_tangent(coef, xi[at], law, self._ensure_tangent_plan(plan), M, **args)

        return _join(self._chunks(cells, chunk_cells, bytes_per_cell, call, sample if load else None), cells=cells)

    def _nonlinear_tail(self, method: str, u, cells, chunk_cells, tail_bytes: int, tail) -> SecantResult:
        """The micro iteration of ``cells`` at ``u`` with what the last ``solve_nonlinear`` kept -- its law, limits, rows, load and the
        history it started from -- and ``tail(b, n)``, the tail arguments of ``plan.secant`` for the n cells from position b, chunk by
        chunk -> the joined ``SecantResult`` with ``cells`` (its ``criterion`` / ``reconstruction`` hold the tail).  One WARNING with
        the counts per status when a cell did not stop with status 0."""
        st = self._nonlinear_state
        if st is None:
            raise RuntimeError(f"{method}(nonlinear=True) evaluates the state a nonlinear solve ended in: call solve_nonlinear() first")
        law = st["law"]
        x = self._macro_dofs(self._or_last_solve(u, method))
        cells = self._cells_argument(cells, method, local=False)
        history = None
        if law.n_history:
            own = self.history_cells
            at = np.searchsorted(own, cells)
            inside = (at < len(own)) & (own[np.minimum(at, len(own) - 1)] == cells)
            if not inside.all():
                raise ValueError(f"{method}(nonlinear=True): the law has history variables and this rank holds the history of the cells "
                                 f"{own[0]} .. {own[-1]} (history_cells) only; cell {int(cells[~inside][0])} is not among them")
            history = st["history"][at]
        xi = self._macro_strains(cells, x)
        rows = st["rows"][cells]
        points = np.ascontiguousarray(self._cell_mesh.cell_midpoints()[:, : self._tdim])
        if st["load"] and self._polarisation is None:
            raise RuntimeError(f"{method}(nonlinear=True): solve_nonlinear ran with load=True and the load has been cleared since: set it again")
        limits = dict(max_iter=st["micro_iter"], tol=st["micro_tol"], relax=st["relax"])
        r = self._secant_chunks(cells, xi, law, rows, points, chunk_cells, history, st["load"], tail_bytes, lambda b, n: dict(limits, **tail(b, n)))
        counts = {int(k): int((r.status == k).sum()) for k in np.unique(r.status)}
        if any(k != 0 for k in counts):
            self._logger.warning("%s(nonlinear=True): not every micro iteration converged; micro cells by status: %s", method,
                                 ", ".join(f"{k}: {n}" for k, n in sorted(counts.items())))
        return r

    def reconstruct(self, u=None, cells=None, fields: bool = False, chunk_cells: int | None = None, regions=None,
                    nonlinear: bool = False) -> Reconstruction:
        """HMM reconstruction of the micro fields in the sampling boxes of ``cells`` (default: every macro cell) from the macro solution
        ``u`` (a macro ``fem.Function`` or its dof array; default: the last ``solve()`` result): R = u_H + corrector of xi_T, with xi_T the
        macro gradient / strain of u on the cell (hommx_reconstruct_source).  Returns a ``Reconstruction`` with ``cells``:
        per-cell mean strain / flux, energy (sum over the cells of vol(T) energy_T is the macro energy u . K_H u), the largest flux and
        where it is reached, and with ``fields`` the per-element strain and flux [N, n_el, t].

        The coefficient crosses the boundary as ``solve()`` sends it (``_coef_stream``): ``TwoPhase`` and ``Separable`` as a few numbers per
        cell, sampled on the device; anything else as element means.  ``regions``: per-region statistics (the ``region_*`` fields: mean
        strain and flux, energy, largest flux of, say, the fibre and the matrix) -- ``True`` (the two phases of a ``TwoPhase``
        coefficient: region 0 outside, 1 inside), integer labels [n_el] of the micro elements, or a callable y -> label evaluated at the
        micro element midpoints; labels from 8 up are in no region.

        The cells are reconstructed in chunks of ``chunk_cells`` (default: about 256 MB of coefficient stream when it is sampled on the
        host, of outputs when it is sampled on the device).  Under a process group this runs on the calling rank alone, for the cells it
        is given: there is no collective.

        ``nonlinear=True`` (after ``solve_nonlinear``): the statistics of the NONLINEAR state -- the micro iteration of
        the asked cells at ``u`` (default: the last result, which after ``solve_nonlinear`` is the nonlinear solution) with that
        call's law, limits and starting history, and the reconstruction of the stream every cell stops on, on the device
        (hommx_secant_state_source).  The result also carries ``secant`` (rounds, change, status per cell).  ``fields`` is not
        offered there (``criterion(crit, nonlinear=True, fields=True)`` returns the state), and a solver that ran
        ``solve_nonlinear(load=True)`` raises ``RuntimeError``: the statistics have no load term.  Without it the call is the linear
        one it was, for the coefficient ``A``."""
        if nonlinear:
            if self._nonlinear_state is not None and self._nonlinear_state["load"]:
                raise RuntimeError("reconstruct(nonlinear=True): solve_nonlinear ran with load=True, and the reconstruction statistics have "
                                   "no load term; criterion(crit, nonlinear=True, fields=True) returns the loaded state")
            if fields:
                raise ValueError("reconstruct(nonlinear=True) returns the statistics; criterion(crit, nonlinear=True, fields=True) returns "
                                 "the strain and the flux of the nonlinear state")
            labels = self._region_labels(regions)
            kw = dict(reconstruct=True, **({} if labels is None else {"regions": labels[0], "n_regions": labels[1]}))
            t = self._tensor_size()
            r = self._nonlinear_tail("reconstruct", u, cells, chunk_cells, 8 * (2 * t + 3 + (labels[1] * (2 * t + 4) if labels else 0)),
                                     lambda b, n: kw)
            out = dataclasses.replace(r.reconstruction, cells=r.cells)
            out.secant = dataclasses.replace(r, criterion=None, reconstruction=None)
            return out
        x = self._macro_dofs(self._or_last_solve(u, "reconstruct"))
        cells = self._cells_argument(cells, "reconstruct", local=False)
        xi = self._macro_strains(cells, x)
        labels = self._region_labels(regions)
        kw = {} if labels is None else {"regions": labels[0], "n_regions": labels[1]}

        def bytes_per_cell():
            n_el, t = self._cell_mesh.num_cells, self._tensor_size()
            if self._sampled_on_device():  # the outputs
                return 8 * (2 * t + 3 + t * t + (labels[1] * (2 * t + 4) if labels else 0) + (2 * n_el * t if fields else 0)) + 4
            return n_el * (1 if self._kind == "poisson" else 2) * 8  # the coefficient stream

        parts = self._chunks(cells, chunk_cells, bytes_per_cell,
                             lambda plan, coef, M, _, sub, b: plan.reconstruct(coef, xi[b:b + len(sub)], M, fields=fields, **kw))
        return _join(parts, xi=xi, cells=cells)

    def load_response(self, cells=None, fields: bool = False, correctors: bool = False, chunk_cells: int | None = None) -> LoadResponse:
        """The response of the sampling boxes of ``cells`` (default: every macro cell) to the polarisation alone (hommx_loads_source with
        a load solve) -> ``LoadResponse`` with ``cells`` and one load: the effective polarisation, the energy of the
        polarisation corrector, the mean and the largest total flux q = P + A eps(chi_P) and where it is reached; with ``fields`` the
        per-element strain and total flux [N, 1, n_el, t], with ``correctors`` the corrector [N, 1, n_nodes * bs].

        By linearity the micro stress under the macro strain of a solution plus the prestress is
        ``reconstruct(...).flux + load_response(...).flux[:, 0]``.  Every micro mesh has the load solve (an unstructured one on the frontal
        route substitutes on its pivot columns).  The cells run in chunks of ``chunk_cells`` (default: 256 MB of sampled loads and outputs).  Under a process group
        this runs on the calling rank alone, for the cells it is given: there is no collective."""
        if self._polarisation is None:
            raise RuntimeError("load_response() needs a polarisation: call set_polarisation() first")
        cells = self._cells_argument(cells, "load_response", local=False)

        def bytes_per_cell():
            n_el, t = self._cell_mesh.num_cells, self._tensor_size()
            n_dof = (int(self._periodic_to_micro_nodes().max()) + 1) * self._bs if correctors else 0
            # doubles per cell: P[n_el, t] | P_eff, energy, stats, A_eff | strain and flux | corrector (info: 4 bytes more)
            return 8 * (n_el * t + (t + 1 + t + 2 + t * t) + (2 * n_el * t if fields else 0) + n_dof) + 4

        return _join(self._load_blocks(cells, chunk_cells, bytes_per_cell, response=True, fields=fields, return_correctors=correctors), cells=cells)

    def criterion(self, crit: Criterion, u=None, cells=None, field_values=None, values: bool = False, fields: bool = False, load=None,
                  chunk_cells: int | None = None, nonlinear: bool = False) -> CriterionResult:
        """A failure criterion ``crit`` (a ``Criterion``: von Mises against a phase-dependent yield stress, a largest principal stress, a
        critical flux, ...) on the micro state ``reconstruct`` forms in the sampling boxes of ``cells`` (default: every macro cell) from
        the macro solution ``u`` (default: the last ``solve()`` result), evaluated ON THE DEVICE where the stress is formed
        (hommx_criterion_source) -> ``CriterionResult`` with ``cells``: per cell the largest value, the element reaching it,
        the mean and the volume fraction at or above ``crit.threshold`` -- four numbers per macro cell cross the boundary.  ``values``:
        the criterion of every element [N, n_el] as well; ``fields``: the strain and flux it saw [N, n_el, t].

        ``load``: None includes the polarisation or eigenstrain when one is set (the physical stress contains it: the criterion sees
        ``reconstruct(...).flux + load_response(...).flux[:, 0]``, sampled as ``load_response`` samples it, on the device where the plan
        takes load sources); False is the mechanical part alone; True insists on the load and raises ``RuntimeError`` without one.
        ``field_values``: the values of the criterion's own fields ``f[k]`` per macro cell, in the shapes ``set_fields`` takes;
        ``RuntimeError`` when the criterion reads fields and they are missing.  In the criterion ``x`` is the macro cell midpoint and
        ``y`` the centroid of the micro element.  The cells run in chunks of ``chunk_cells`` (default: about 256 MB of what crosses the
        boundary).  Under a process group this runs on the calling rank alone, for the cells it is given: there is no collective.

        ``nonlinear=True`` (after ``solve_nonlinear``): the criterion on the NONLINEAR state -- the micro iteration of the
        asked cells at ``u`` (default: the last result, which after ``solve_nonlinear`` is the nonlinear solution) with that call's
        law, limits, starting history and, where it ran with ``load=True``, the solver's load, and the criterion on the stream every
        cell stops on, on the device (hommx_secant_state_source): no stream crosses the boundary.  There ``c[k]`` is the softened
        coefficient, ``b[k]`` the base one (the solver's ``A``) and ``h[k]`` the history at the start of the load step
        (``Criterion(..., history=law.n_history)``), before or after ``commit_history()``.  The result also carries ``secant``
        (rounds, change, status per cell); one WARNING when a cell did not stop with status 0.  ``load`` must stay None: the load of
        the nonlinear run is part of its state.  A criterion that reads ``b`` or ``h`` needs ``nonlinear=True``.  Under a process
        group the cells of a law with history must be among ``history_cells``."""
        if nonlinear:
            if load is not None:
                raise ValueError("criterion(nonlinear=True) takes no load=: the load of the nonlinear run is part of its state "
                                 "(solve_nonlinear(load=True) decides it)")
            if crit.n_fields and field_values is None:
                raise RuntimeError(f"the criterion reads the fields {', '.join(crit.field_names)}: pass field_values, their values per macro cell")
            if self._nonlinear_state is not None and crit.n_history and crit.n_history != self._nonlinear_state["law"].n_history:
                raise ValueError(f"the criterion declares history={crit.n_history}; the law of solve_nonlinear has "
                                 f"{self._nonlinear_state['law'].n_history} history variables")
            crit_rows = self._msh.cell_midpoints()
            if crit.n_fields:
                crit_rows = np.concatenate([crit_rows, self._field_values(crit, field_values)], axis=1)
            n_el, t = self._cell_mesh.num_cells, self._tensor_size()
            picked = self._cells_argument(cells, "criterion", local=False)
            r = self._nonlinear_tail("criterion", u, picked, chunk_cells, 8 * (4 + (n_el if values else 0) + (2 * n_el * t if fields else 0)),
                                     lambda b, n: dict(criterion=crit, crit_rows=crit_rows[picked[b:b + n]], crit_values=values,
                                                       crit_fields=fields))
            out = dataclasses.replace(r.criterion, cells=r.cells)
            out.secant = dataclasses.replace(r, criterion=None, reconstruction=None)
            return out
        if crit.reads_state:
            names = ", ".join(f"{n}[{crit.state_indices[n] - 1}]" for n in "bh" if crit.state_indices[n])
            raise ValueError(f"the criterion reads {names}, the nonlinear state: pass nonlinear=True (after solve_nonlinear)")
        if load is True and self._polarisation is None:
            raise RuntimeError("criterion(load=True) needs a polarisation: call set_polarisation() or set_eigenstrain() first")
        if crit.n_fields and field_values is None:
            raise RuntimeError(f"the criterion reads the fields {', '.join(crit.field_names)}: pass field_values, their values per macro cell")
        x = self._macro_dofs(self._or_last_solve(u, "criterion"))
        cells = self._cells_argument(cells, "criterion", local=False)
        xi = self._macro_strains(cells, x)
        rows = self._msh.cell_midpoints()[cells]
        if crit.n_fields:
            rows = np.concatenate([rows, self._field_values(crit, field_values)[cells]], axis=1)
        points = np.ascontiguousarray(self._cell_mesh.cell_midpoints()[:, : self._tdim])  # where _region_labels evaluates a callable
        with_load = self._polarisation is not None and load is not False

        def bytes_per_cell():
            n_el, t = self._cell_mesh.num_cells, self._tensor_size()
            out = 8 * (4 + t * t + (n_el if values else 0) + (2 * n_el * t if fields else 0)) + 4
            if with_load and not isinstance(self._polarisation, Expression):
                out += 8 * n_el * t  # a sampled load
            return out if self._sampled_on_device() else out + n_el * (1 if self._kind == "poisson" else 2) * 8

        def call(plan, coef, M, P, sub, b):
            kw = {} if P is None else {"P": P[0], "per_cell": P[1], "eigenstrain": P[2]}
            return plan.criterion(coef, xi[b:b + len(sub)], crit, M, rows=rows[b:b + len(sub)], points=points, values=values, fields=fields, **kw)

        parts = self._chunks(cells, chunk_cells, bytes_per_cell, call, (lambda sub, kind: self._polarisation_loads(sub, kind)) if with_load else None)
        return _join(parts, cells=cells)

    def _ensure_tangent_plan(self, plan):
        """The sibling plan of ``plan``'s tangent kind on the same micro mesh and device, built on first use and kept (a stale one
        is closed), and reserved for as many cells as ``plan`` is: ``_ensure_plan`` passes every later reservation on."""
        tp = self._tangent_plan
        if tp is None or tp.kind != plan.tangent_kind:
            if tp is not None:
                tp.close()
            if self._n_micro is None:
                tp = MicroCellPlan.from_mesh(self._cell_mesh, plan.tangent_kind, device=plan.device)
            else:
                tp = MicroCellPlan(self._tdim, self._n_micro, plan.tangent_kind, device=plan.device)
            self._tangent_plan, self._tangent_reserved = tp, 0
        if self._reserved_cells > self._tangent_reserved:
            tp.reserve(self._reserved_cells)
            self._tangent_reserved = self._reserved_cells
        return tp

    def _secant_tensors(self, cells: np.ndarray, xi: np.ndarray, law: SecantLaw, rows: np.ndarray, points: np.ndarray, chunk_cells,
                        tangent: bool = False, history: np.ndarray | None = None, load: bool = False, **kw) -> SecantResult:
        """``plan.secant`` of ``law`` on ``cells`` under the macro strains ``xi``, chunk by chunk -> one ``SecantResult`` with ``cells``;
        ``tangent``: ``plan.secant_tangent`` on the sibling plan instead, with ``tangent`` and ``asymmetry``.  Under a process group
        every rank iterates its block and one all-gather of t t + t + 3 numbers per cell (2 t t + t + 4 with the tangent; and the info
        flags) returns the fields to every rank, as ``_effective_polarisation`` does.  ``history``: the history variables of THIS
        RANK'S block of ``cells`` (all of them without a process group), passed to the plan chunk by chunk; what the plan returns for
        the block goes to ``history_trial`` and is not gathered.  ``load``: the polarisation or the eigenstrain of the solver enters
        every round (``plan.secant(P=...)``), sampled chunk by chunk as ``criterion()`` samples it -- an ``Expression`` as
        its program where the plan takes load sources; an eigenstrain crosses AS IT IS, since its eigenstress belongs to the
        current stream of every round."""
        t = self._tensor_size()

        def local(b, e):
            r = self._secant_chunks(cells[b:e], xi[b:e], law, rows[b:e], points, chunk_cells, history, load, 8 * (t * t + 1) if tangent else 0,
                                    lambda at, n: kw, tangent)
            if history is not None:
                self.history_trial = r.history
            return r

        if not self._sharded():
            return local(0, len(cells))
        from .dist import run_sharded

        def block(b, e):
            r = local(b, e)
            more = [r.tangent.reshape(e - b, t * t), r.asymmetry[:, None]] if tangent else []
            return np.concatenate([r.A_eff.reshape(e - b, t * t), r.mean_flux, r.rounds[:, None], r.change[:, None], r.status[:, None]] + more,
                                  axis=1), r.info

        width = t * t + t + 3
        packed, info = run_sharded(t, len(cells), block, device=self._shard_device(), shape=(width + (t * t + 1 if tangent else 0),))
        out = SecantResult(packed[:, :t * t].reshape(-1, t, t).copy(), packed[:, t * t:t * t + t].copy(),
                           np.rint(packed[:, width - 3]).astype(np.int64), packed[:, width - 2].copy(),
                           np.rint(packed[:, width - 1]).astype(np.int64), info, cells=cells)
        if tangent:
            out.tangent, out.asymmetry = packed[:, width:width + t * t].reshape(-1, t, t).copy(), packed[:, -1].copy()
        return out

    def solve_nonlinear(self, law: SecantLaw, max_iter: int = 30, tol: float = 1e-8, micro_iter: int = 50, micro_tol: float = 1e-10,
                        relax: float = 1.0, field_values=None, u0=None, chunk_cells: int | None = None, method: str = "secant",
                        load: bool = False) -> fem.Function:
        """The two-scale problem with a strain-dependent micro coefficient ``law`` (a ``SecantLaw``: the entries of the coefficient of a
        micro element as expressions of its own strain ``e``, secant stress ``s`` and base coefficient ``c``, the solver's ``A``), by
        the Kacanov (secant) iteration on both scales.  u^0 is ``u0`` (a macro ``fem.Function`` or its dof array) or
        ``solve()``.  Per macro step: the macro strain of u^k on every cell, the secant iteration of every sampling box ON THE DEVICE
        (hommx_secant_source: at most ``micro_iter`` rounds to ``micro_tol``, relaxed by ``relax``), the macro matrix from the secant
        tensors, and the macro solve of ``solve()`` on it.  It stops when ``max |u^{k+1} - u^k| <= tol max |u^{k+1}|``, or after
        ``max_iter`` steps.  ``field_values``: the values of the law's own fields ``f[k]`` per macro cell, in the shapes ``set_fields``
        takes.  In the law ``x`` is the macro cell midpoint and ``y`` the centroid of the micro element.

        Afterwards ``effective_tensors`` holds the secant tensors of the last step, ``secant`` its ``SecantResult`` (rounds, change,
        status, info and mean flux per cell), ``nonlinear_history`` the relative macro change of every step; the solver is marked for
        reassembly, so a later ``solve()`` is the linear one again.  One WARNING when the macro loop or any cell did not converge.

        ``method="newton"`` (an explicit law, ``law.explicit``): per step the micro iteration of every box and, at the
        state it stops in, the consistent tangent D_T = d sigma_T / d xi on a sibling plan of the tangent kind (hommx_secant_tangent_source;
        the solver builds and keeps that plan); the macro matrix comes from D_T and the load from P_T = sigma_T - D_T xi_T, which enters
        ``solve()`` where an effective polarisation does, so u^{k+1} solves the linearisation sigma_T + D_T (xi - xi_T): Newton's step,
        with the same stopping rule and the same ``nonlinear_history``.  ``effective_tensors`` holds the secant tensors,
        ``tangent_tensors`` D (NaN for a cell of status 2 or 3: such a cell enters the step with its secant tensor and no load, as it
        does under ``"secant"``, and the status WARNING counts it).  One WARNING when the largest ``asymmetry`` exceeds 1e-8: the law then has no potential and the steps
        are quasi-Newton steps with the symmetric part of the tangent.

        ``load=True``: the polarisation or the eigenstrain of the solver (``set_polarisation`` / ``set_eigenstrain``, a
        device-sampled ``Expression`` with its ``set_polarisation_fields`` included) enters every micro iteration
        (hommx_secant_load_source): every round of every box ends in a load solve on its current stream.  Beside a polarisation the
        law reads the total strain and the total flux; beside an eigenstrain the elastic strain ``e - E`` and ``material . (e - E)``:
        thermal damage, swelling, prestress in a softening matrix.  In BOTH methods the macro step then takes its load from
        P_T = sigma_T - matrix xi_T, as Newton does: for ``"secant"`` the matrix is the secant tensor and P_T the effective
        polarisation of the secant state.  Afterwards ``effective_polarisation`` holds mean_flux - A_eff xi of the last step.
        ``RuntimeError`` naming the two setters when nothing is set.  With ``load=False`` and a polarisation set the call raises
        ``RuntimeError`` (pass ``load=True``): a load is never dropped silently.

        ``RuntimeError`` as well when the law reads fields without
        ``field_values``, or ``method="newton"`` meets a law that reads ``s[k]`` (the tangent of an implicit law is out of scope).
        A law with history variables (``SecantLaw(history=[...])``) reads ``self.history[cells, n_el, n_history]``, created
        from ``law.history_initial`` on first use: every macro step passes that same frozen state to the plan (``h[k]`` is the state
        at the start of the LOAD STEP, not of a macro step), and the updates of the last step are left in ``self.history_trial``.
        ``commit_history()`` makes the trial the state -- call it once a load step is accepted --, ``reset_history()`` clears or sets
        it; without a commit a second call reproduces the first.  ``RuntimeError`` naming ``reset_history`` when the state belongs to
        a law with another number of history variables or to another micro mesh.  Both methods are supported.  Under a process group
        every rank keeps the history of its own block of cells only (``history_cells``, the block rule of ``run_sharded``); nothing
        of it is gathered.  In this version the solver holds the history on the HOST: ``n_el n_history`` doubles per cell cross the
        boundary in each direction per macro step (DESIGN 4.17 has the measured cost); ``MicroCellPlan.secant_device`` keeps it
        resident for callers who drive the plan themselves.

        ``criterion(crit, nonlinear=True)`` and ``reconstruct(nonlinear=True)`` evaluate the state this call ended in:
        the solver keeps the law, the micro limits, the law's field rows, ``load`` and a reference to the history the step started
        from.

        Out of scope: warm starts of the micro iteration
        across macro steps (``MicroCellPlan.secant(coef_start=...)`` has them).  Under a process group every rank
        iterates its block of the cells, as in ``solve()``."""
        if self._polarisation is not None and not load:
            raise RuntimeError("solve_nonlinear() does not take the polarisation or eigenstrain that is set unless it is told to: pass "
                               "load=True to solve with it, or clear it (set_polarisation(None))")
        if load and self._polarisation is None:
            raise RuntimeError("solve_nonlinear(load=True) needs a load: call set_polarisation() or set_eigenstrain() first")
        if law.n_fields and field_values is None:
            raise RuntimeError(f"the law reads the fields {', '.join(law.field_names)}: pass field_values, their values per macro cell")
        if method not in ("secant", "newton"):
            raise ValueError(f"method must be 'secant' or 'newton'; got {method!r}")
        newton = method == "newton"
        if newton and not law.explicit:
            raise RuntimeError(f"solve_nonlinear(method='newton') takes an explicit law; this one reads s[{law.state_indices['s'] - 1}] "
                               "(the tangent of an implicit law is out of scope): use method='secant'")
        cells = np.arange(self._msh.num_cells)
        rows = self._msh.cell_midpoints()[cells]
        if law.n_fields:
            rows = np.concatenate([rows, self._field_values(law, field_values)[cells]], axis=1)
        points = np.ascontiguousarray(self._cell_mesh.cell_midpoints()[:, : self._tdim])
        state = self._history_state(law) if getattr(law, "n_history", 0) else None
        u = self._macro_dofs(u0, "u0").copy() if u0 is not None else self.solve().x.array.copy()
        history, converged, result = [], False, None
        for _ in range(int(max_iter)):
            xi = self._macro_strains(cells, u)
            result = self._secant_tensors(cells, xi, law, rows, points, chunk_cells, tangent=newton, history=state, load=load,
                                          max_iter=micro_iter, tol=micro_tol, relax=relax)
            matrix = result.A_eff
            lost = (result.status >= 2)[:, None, None]
            if newton:  # a cell without a state to linearise at (status 2, 3: its tangent is NaN) takes the secant step, as "secant" does
                matrix = np.where(lost, result.A_eff, result.tangent)
                self.tangent_tensors = result.tangent
            if newton or load:  # the constant part of the linearised response; beside a load also under "secant": its effective polarisation
                self._linearisation_load = np.where(lost[:, :, 0], 0.0, result.mean_flux - np.einsum("cmn,cn->cm", matrix, xi))
            self._set_macro_matrix(self._local_stiffness_from_tensors(cells, matrix))
            self.effective_tensors, self.cell_info = result.A_eff, result.info
            self._nonlinear_load = bool(load)
            try:
                new = self.solve().x.array.copy()
            finally:
                self._linearisation_load, self._nonlinear_load = None, False
            if load:
                self.effective_polarisation = result.mean_flux - np.einsum("cmn,cn->cm", result.A_eff, xi)
            change, scale = float(np.abs(new - u).max()), float(np.abs(new).max())
            history.append(change / scale if scale > 0.0 else 0.0)
            u = new
            if change <= tol * scale:
                converged = True
                break
        self.secant, self.nonlinear_history = result, history
        # `state` is the array the step started from: commit_history() rebinds self.history and mutates nothing, so the reference
        # survives a commit and costs no copy
        self._nonlinear_state = dict(law=law, micro_iter=micro_iter, micro_tol=micro_tol, relax=relax, rows=rows, load=bool(load), history=state)
        self._needs_reassembly = True
        counts = {int(s): int((result.status == s).sum()) for s in np.unique(result.status)} if result is not None else {}
        if not converged or any(s != 0 for s in counts):
            self._logger.warning(
                "solve_nonlinear: %s after %d macro steps (last relative change %.3e, tol %.3e); micro cells by status: %s",
                "the macro loop did not converge" if not converged else "the macro loop converged, but not every cell did", len(history),
                history[-1] if history else float("nan"), tol, ", ".join(f"{s}: {n}" for s, n in sorted(counts.items())))
        worst = float(np.nanmax(result.asymmetry, initial=0.0)) if newton and result is not None else 0.0
        if worst > 1e-8:
            self._logger.warning(
                "solve_nonlinear: the element tangents of the law are not symmetric (largest asymmetry %.3e): the law has no potential, "
                "and the macro steps were quasi-Newton steps with the symmetric part of the tangent", worst)
        return self._u

    # -- the history variables of a law -----------------------------------------------------------------------------------
    @property
    def history_cells(self) -> np.ndarray:
        """The macro cells whose history this rank holds, in the order of ``history``'s first axis: all of them, or this rank's block
        under a process group (the block rule of ``run_sharded``)."""
        return self._local_cells()

    def _history_state(self, law: SecantLaw) -> np.ndarray:
        """``self.history`` for ``law``, created from ``law.history_initial`` on first use."""
        shape = (self._local_cell_count(), self._cell_mesh.num_cells, int(law.n_history))
        if self.history is None:
            self.history = np.ascontiguousarray(np.broadcast_to(law.history_initial, shape))
        elif self.history.shape != shape:
            raise RuntimeError(f"the history has shape {self.history.shape}; this law on this micro mesh has (cells, n_el, n_history) = {shape}: "
                               "reset_history() starts a new one")
        return self.history

    def commit_history(self):
        """The history the last ``solve_nonlinear`` left (``history_trial``) becomes the state (``history``): the load step is
        accepted.  ``RuntimeError`` when there is none."""
        if self.history_trial is None:
            raise RuntimeError("commit_history(): no solve_nonlinear() of a law with history variables has run since the last reset_history()")
        self.history = self.history_trial

    def reset_history(self, values=None):
        """Forget the history and the trial (the next ``solve_nonlinear`` starts from ``law.history_initial``), or set the state to
        ``values[len(history_cells), n_el, n_history]`` (``[len(history_cells), n_el]``: one variable)."""
        self.history = self.history_trial = None
        if values is None:
            return
        v = np.array(values, dtype=np.float64, order="C")
        if v.ndim == 2:
            v = v[:, :, None]
        lead = (self._local_cell_count(), self._cell_mesh.num_cells)
        if v.ndim != 3 or v.shape[:2] != lead or not 1 <= v.shape[2]:
            raise ValueError(f"values has shape {np.shape(values)}; expected {lead + ('n_history',)}")
        self.history = v

    def _parameter_directions(self) -> tuple[tuple, np.ndarray]:
        """(names, directions[n_dirs, n_el(, n_comp)]) of the parameters of a ``TwoPhase`` or affine ``Separable`` coefficient: the element
        stream is linear in them, so its derivative with respect to each is one direction every macro cell shares.  ``TwoPhase``: the
        outside and the inside value of every component -- the indicator of each phase; affine: a and b of every component -- 1 and the
        table of g.  Elasticity: the components are (lambda, mu)."""
        co = self._coeff
        if isinstance(co, TwoPhase):
            inside = self._phase_mask().astype(float)
            basis, labels = [1.0 - inside, inside], ["outside", "inside"]
        elif isinstance(co, Separable) and co.family == "affine":
            yq, w = self._quadrature_points()
            table = np.asarray(co.table(yq, w), dtype=float)
            basis, labels = [np.ones_like(table), table], ["a", "b"]
        else:
            raise ValueError("the coefficient has no parameters the element stream is linear in (a TwoPhase or an affine Separable has): "
                             "pass directions=[dA_0, ...], callables (x, y) of the coefficient's shape")
        if self._kind == "poisson":
            return tuple(labels), np.stack(basis)
        comps = ("lambda", "mu")
        unit = np.eye(2)
        if isinstance(co, TwoPhase):  # the order of the values [2][n_comp]
            pairs = [(b, q) for b in range(2) for q in range(2)]
        else:  # the order of the params [n_comp][2]
            pairs = [(b, q) for q in range(2) for b in range(2)]
        return (tuple(f"{labels[b]}.{comps[q]}" for b, q in pairs), np.stack([basis[b][:, None] * unit[q][None, :] for b, q in pairs]))

    def tensor_derivatives(self, cells=None, directions=None, chunk_cells: int | None = None) -> Sensitivities:
        """Derivatives of A_H / C_H of ``cells`` (default: this rank's macro cells) with respect to the micro coefficient
        (hommx_sensitivity_source) -> ``Sensitivities`` with ``names``, ``dA[N, n_dirs, t, t]``, ``A_eff``, ``info`` and ``cells``.

        Without ``directions`` the derivatives are those with respect to the parameters of the coefficient: the outside and the inside
        value of a ``TwoPhase`` coefficient, a and b of an affine ``Separable`` one, of every component (lambda and mu for the elasticity
        classes), and the named parameters ``p[k]`` of an ``Expression`` (``Expression(..., p=[...], parameter_names=...)``): the
        program is differentiated on the device in forward mode, in the pass that samples it, so nothing is sampled on the host and no
        direction stream crosses the boundary.  The fields ``f[k]`` of an ``Expression`` (``fields=...``, ``set_fields``) follow the
        parameters: ``names == parameter_names + field_names`` and ``dA[N, n_params + n_fields, t, t]``, where the field entry of cell
        T is the derivative with respect to T's OWN value (the tensor of a cell does not depend on another cell's).  Any other coefficient raises ``ValueError``: its element stream is not linear in a few
        parameters.
        ``directions=[dA_0, ...]``: callables (x, y) of the coefficient's shape, up to 8; each is sampled exactly as the coefficient is
        (the same quadrature degree and packing) and dA[:, k] is the derivative of A_H along it.

        The coefficient crosses the boundary as ``solve()`` sends it (``_coef_stream``).  The cells run in chunks of ``chunk_cells``
        (default: about 256 MB of coefficient and direction streams).  Under a process group this runs on the calling rank alone:
        there is no collective."""
        names, cells, parts = self._direction_blocks("tensor_derivatives", cells, directions, chunk_cells,
                                                     lambda plan, coef, M, **kw: plan.sensitivities(coef, M, **kw))
        return _join(parts, grad=None, names=names, cells=cells)

    def _direction_blocks(self, what: str, cells, directions, chunk_cells: int | None, call, curvature: bool = False) -> tuple[tuple, np.ndarray, list]:
        """(names, cells, results) of ``call(plan, coef, M, directions=..., per_cell=...)`` over ``cells`` (default: this rank's macro
        cells) in chunks of ``chunk_cells``: the cells, names and directions of ``tensor_derivatives`` and ``tensor_second_derivatives``.
        ``curvature``: the parameter directions of a device-sampled ``Expression`` with the curvature term, for any ``p_degree``
        (``call`` then also takes ``curvature=True``); every other coefficient raises ``ValueError``."""
        cells = self._cells_argument(cells, what, local=True)
        self._cell_rows(cells[:1])  # an Expression whose fields are not set: the RuntimeError that names set_fields, before anything else
        names, shared, directions = self._directions(what, directions, curvature)
        more = {"curvature": True} if curvature else {}

        def sample(sub, kind):  # the caller's directions on a chunk, each sampled as the coefficient is
            if shared is not None:
                return shared
            sampled = [self._element_means(sub, f) for f in directions]
            if any(k != kind for _, k in sampled):
                raise ValueError(f"every direction must have the coefficient's shape (plan kind {kind!r}); got {[k for _, k in sampled]}")
            return np.stack([d for d, _ in sampled], axis=1)

        streams = 1 + (len(directions) if shared is None else 0)  # the parameter tangents never cross the boundary
        parts = self._chunks(cells, chunk_cells, lambda: 8 * self._cell_mesh.num_cells * (1 if self._kind == "poisson" else 2) * streams,
                             lambda plan, coef, M, dirs, sub, b: call(plan, coef, M, directions=dirs, per_cell=shared is None, **more), sample)
        return names, cells, parts

    def _directions(self, what: str, directions, curvature: bool) -> tuple[tuple, object, list | None]:
        """(names, shared, callables) of the directions of ``_direction_blocks``.  ``shared``: the directions every cell shares
        [n_dirs, n_el(, n_comp)] (``_parameter_directions``), ``"parameters"`` (the parameter tangents of a device-sampled
        ``Expression``), or None: ``callables``, the caller's ``directions``, are sampled cell by cell."""
        co = self._coeff
        if directions is None and isinstance(co, Expression) and (co.n_params or co.n_fields) and self._sampled_on_device() == "solve_program":
            # the parameter tangents of the program, formed on the device with the stream: nothing is sampled, no direction stream is sent
            if what == "tensor_second_derivatives" and not co.affine_in_parameters and not curvature:
                raise ValueError(
                    f"the expression is not affine in its parameters (p_degree {co.p_degree}): the Hessian of A_H also needs dA_H along "
                    "d2A/dp_a dp_b, the curvature term.  Pass curvature=True: the library then forms those streams on the device in "
                    "second-order forward mode and d2A is the whole Hessian.  directions=[...] with your own streams remains available: "
                    "the second derivatives along them")
            names, shared = co.parameter_names + co.field_names, "parameters"
        elif curvature:
            if directions is not None:
                why = "directions=[...] are the caller's own streams, whose second derivatives the library cannot know"
            elif not isinstance(co, Expression):
                why = f"the coefficient is a {type(co).__name__}, not an Expression (TwoPhase and Separable are affine: their curvature term is zero)"
            elif not (co.n_params or co.n_fields):
                why = "the Expression has neither parameters (p=[...]) nor fields (fields=...)"
            else:
                why = "the Expression is sampled on the host here, and the second-order tangents are formed by the device sampler only"
            raise ValueError(f"curvature=True needs a device-sampled Expression with parameters or fields: {why}")
        elif directions is None:
            names, shared = self._parameter_directions()
        else:
            directions = list(directions)
            names, shared = tuple(getattr(f, "__name__", f"direction{k}") for k, f in enumerate(directions)), None
        return names, shared, directions

    def energy_derivatives(self, u=None, v=None, **kw) -> np.ndarray:
        """[N, n_dirs]: vol(T)/vol(Y) xi_v(T) . dA_H[d](T) xi_u(T) for the cells and directions of ``tensor_derivatives(**kw)``, with xi the
        macro gradient / Voigt strain ``reconstruct()`` forms -- the contribution of macro cell T to d(v . K_H u)/d theta_d at frozen u, v:
        the compliance gradient for v = u (the default; ``u`` defaults to the last ``solve()`` result), the adjoint product otherwise.
        For a field ``f[k]`` of an ``Expression`` only cell T depends on the value of T, so entry ``[T, n_params + k]`` is the WHOLE
        derivative of u . K_H u at frozen u with respect to the design variable (T, k), not one contribution among many."""
        u = self._or_last_solve(u, "energy_derivatives")
        td = self.tensor_derivatives(**kw)
        xv, xu, vol = self._energy_weights(td.cells, u, v)
        return vol[:, None] * np.einsum("cm,cdmn,cn->cd", xv, td.dA, xu)

    def _energy_weights(self, cells: np.ndarray, u, v) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(xi_v[N, t], xi_u[N, t], vol(T)/vol(Y)[N]) of ``cells``: the macro gradient / Voigt strain of the macro fields (``v`` None: u)."""
        xi = lambda f: self._macro_strains(cells, self._macro_dofs(f, "the macro field"))
        xu = xi(u)
        return (xu if v is None else xi(v)), xu, self._volume_ratio(cells)

    def tensor_second_derivatives(self, cells=None, directions=None, chunk_cells: int | None = None,
                                  curvature: bool = False) -> SecondSensitivities:
        """Second derivatives of A_H / C_H of ``cells`` (default: this rank's macro cells) with respect to the micro coefficient
        (hommx_second_sensitivity_source) -> ``SecondSensitivities`` with ``names``, ``d2A[N, n_dirs, n_dirs, t, t]``, the
        first derivatives ``dA[N, n_dirs, t, t]`` of the same call, ``A_eff``, ``info`` and ``cells``.

        Names and directions are those of ``tensor_derivatives``: without ``directions`` the parameters of a ``TwoPhase`` or an affine
        ``Separable`` coefficient or of an ``Expression`` that is affine in its parameters (``affine_in_parameters``: the curvature term
        vanishes and d2A is the exact Hessian; one that is not raises ``ValueError``, as any other coefficient does), else up to 8
        callables (x, y) of the coefficient's shape.
        d2A[:, a, b] is exact on the discrete problem -- the Hessian of A_H a Newton or Gauss-Newton step needs, with no step size to
        tune -- and costs one load solve per direction, on every micro mesh.  The cells run in chunks of ``chunk_cells``.  Under a process
        group this runs on the calling rank alone: there is no collective.

        ``curvature=True`` (a device-sampled ``Expression`` with parameters or fields, without ``directions``): the whole Hessian of A_H
        in the parameters and fields for ANY expression -- a radius inside ``tanh``, ``p[0]*p[1]``, a parameter in a denominator.  The
        device pass that samples the program carries second-order tangents, and d2A[:, a, b] also takes dA_H along d2 coef / dp_a dp_b
        (hommx_expand_second_tangents, HOMMX_DIRS_PARAMETERS_CURVATURE).  For an affine expression that term is +0.0 and the result is
        the default call's; any other coefficient, ``directions=[...]`` or a host-sampled expression raises ``ValueError``."""
        names, cells, parts = self._direction_blocks("tensor_second_derivatives", cells, directions, chunk_cells,
                                                     lambda plan, coef, M, **kw: plan.second_sensitivities(coef, M, first=True, **kw),
                                                     curvature=curvature)
        return _join(parts, names=names, cells=cells)

    def energy_second_derivatives(self, u=None, v=None, **kw) -> np.ndarray:
        """[N, n_dirs, n_dirs]: vol(T)/vol(Y) xi_v(T) . d2A_H[a][b](T) xi_u(T) for the cells and directions of
        ``tensor_second_derivatives(**kw)`` -- the contribution of macro cell T to the second derivative of v . K_H u at FROZEN u, v
        (``u`` defaults to the last ``solve()`` result, ``v`` to u).  The response of u itself to the parameters (the du/dtheta terms of a
        compliance or misfit Hessian) is the caller's macro solve: it needs ``energy_derivatives`` and K_H, not the cell problems."""
        u = self._or_last_solve(u, "energy_second_derivatives")
        td = self.tensor_second_derivatives(**kw)
        xv, xu, vol = self._energy_weights(td.cells, u, v)
        return vol[:, None, None] * np.einsum("cm,cabmn,cn->cab", xv, td.d2A, xu)

    def _stratification_parameters(self, cells: np.ndarray, parameters) -> tuple[tuple, np.ndarray]:
        """(names, dM[N, n_params, d, d]) of the design parameters of the stratification: every entry of ``parameters`` is a callable
        x -> [d, d], the derivative of ``Dtheta_transpose`` with respect to one parameter, evaluated as ``_stratification`` evaluates M."""
        parameters = list(parameters)
        if not parameters:
            raise ValueError("parameters must hold at least one callable x -> [d, d]")
        names = tuple(getattr(f, "__name__", f"parameter{k}") for k, f in enumerate(parameters))
        return names, np.stack([self._matrix_at_midpoints(f, cells, f"parameters[{k}]") for k, f in enumerate(parameters)], axis=1)

    def _stratification_blocks(self, cells: np.ndarray, chunk_cells: int | None, weights=None, full: bool = True) -> list:
        """``plan.stratification_sensitivities`` of ``cells`` in chunks of ``chunk_cells`` (default: about 256 MB of coefficient stream
        and outputs); the coefficient crosses the boundary as ``solve()`` sends it."""
        d, t = self._tdim, self._tensor_size()
        return self._chunks(cells, chunk_cells,
                            lambda: 8 * (self._cell_mesh.num_cells * (1 if self._kind == "poisson" else 2) + d * d * (t * t if full else 1) + 2 * t * t) + 4,
                            lambda plan, coef, M, _, sub, b: plan.stratification_sensitivities(
                                coef, M, weights=None if weights is None else weights[b:b + len(sub)], full=full))

    def stratification_derivatives(self, cells=None, parameters=None, chunk_cells: int | None = None) -> StratSensitivities:
        """Derivatives of A_H / C_H of ``cells`` (default: this rank's macro cells) with respect to the stratification M = Dtheta^T(c_T)
        (hommx_stratification_sensitivity_source) -> ``StratSensitivities`` with ``dA_dM[N, d, d, t, t]``, ``A_eff``, ``info``
        and ``cells``.  A class without stratification differentiates at M = I.

        ``parameters=[dM_0, ...]``: callables x -> [d, d], the derivative of ``Dtheta_transpose`` with respect to a design parameter (a
        fibre angle, a curvature), evaluated as ``Dtheta_transpose`` itself is; the result then also carries ``names`` and
        ``dA[N, n_params, t, t]`` = sum_ab dM_p[a, b] dA_dM[:, a, b], the derivative of A_H along each parameter (formed on the host).

        The cells run in chunks of ``chunk_cells``.  Under a process group this runs on the calling rank alone: there is no collective."""
        cells = self._cells_argument(cells, "stratification_derivatives", local=True)
        out = _join(self._stratification_blocks(cells, chunk_cells), grad_M=None, cells=cells)
        if parameters is not None:
            out.names, dM = self._stratification_parameters(cells, parameters)
            out.dA = np.einsum("cpab,cabmn->cpmn", dM, out.dA_dM)
        return out

    def stratification_energy_derivatives(self, u=None, v=None, cells=None, parameters=None) -> np.ndarray:
        """[N, d, d]: vol(T)/vol(Y) sum_mn xi_v(T)[m] dA_H[m, n]/dM(T) xi_u(T)[n] for ``cells`` (default: this rank's macro cells), with xi
        the macro gradient / Voigt strain ``reconstruct()`` forms -- the derivative of the contribution of macro cell T to v . K_H u with
        respect to its M at frozen u, v: the compliance gradient for v = u (the default; ``u`` defaults to the last ``solve()`` result),
        the adjoint product otherwise.  The weights xi_v (x) xi_u go to the device, only d d numbers per cell come back.  With
        ``parameters`` (as ``stratification_derivatives`` takes them) the result is contracted with them: [N, n_params]."""
        u = self._or_last_solve(u, "stratification_energy_derivatives")
        cells = self._cells_argument(cells, "stratification_energy_derivatives", local=True)
        xv, xu, vol = self._energy_weights(cells, u, v)
        parts = self._stratification_blocks(cells, None, weights=np.einsum("cm,cn->cmn", xv, xu), full=False)
        grad = vol[:, None, None] * np.concatenate([r.grad_M for r in parts])
        if parameters is None:
            return grad
        return np.einsum("cpab,cab->cp", self._stratification_parameters(cells, parameters)[1], grad)

    def plot_solution(self, u=None):  # hmm.py:493-511 (visualisation: out of scope)
        raise NotImplementedError("plotting is out of scope of hommx_amd; use u.x.array with any plotting tool")


def _zero_rows_columns(A: sp.csr_matrix, idx: np.ndarray) -> sp.csr_matrix:
    """PETSc MatZeroRowsColumns(idx, diag=1.0) (hmm.py:478)."""
    n = A.shape[0]
    keep = np.ones(n)
    keep[idx] = 0.0
    Dk = sp.diags(keep)
    A = Dk @ A @ Dk
    return (A + sp.diags(1.0 - keep)).tocsr()


def _box_boundary_nodes(msh: Mesh) -> np.ndarray:
    x = msh.geometry.x[:, : msh.topology.dim]
    lo, hi = x.min(axis=0), x.max(axis=0)
    return np.nonzero(np.any(np.isclose(x, lo) | np.isclose(x, hi), axis=1))[0]


class PoissonHMM(BaseHMM):
    """hmm.py:514-667.  Forms: micro LHS :644-647, RHS :649-650, local stiffness :652-667."""

    _kind = "poisson"

    def __init__(self, msh, A, f, msh_micro, eps, petsc_options_global_solve=None, petsc_options_cell_problem=None,
                 petsc_options_prefix: str = "hommx_PoissonHMM", **kw):
        super().__init__(msh, A, f, msh_micro, eps, petsc_options_global_solve, petsc_options_cell_problem,
                         petsc_options_prefix, **kw)
        # homogeneous Dirichlet on the bounding box by default (hmm.py:598-636)
        self._bcs = [fem.dirichletbc(0.0, _box_boundary_nodes(self._msh), self._V_macro)]

    def _setup_macro_function_space(self):
        return fem.functionspace(self._msh, ("Lagrange", 1))


class PoissonStratifiedHMM(PoissonHMM):
    """hmm.py:670-789: ``Dtheta_transpose`` comes right after ``eps`` (hmm.py:717-728); M[i][j] = d theta_j/d x_i."""

    def __init__(self, msh, A, f, msh_micro, eps, Dtheta_transpose, petsc_options_global_solve=None,
                 petsc_options_cell_problem=None, petsc_options_prefix: str = "hommx_PoissonStratifiedHMM", **kw):
        super().__init__(msh, A, f, msh_micro, eps, petsc_options_global_solve, petsc_options_cell_problem,
                         petsc_options_prefix, **kw)
        self._Dtheta_t = Dtheta_transpose


class LinearElasticityHMM(BaseHMM):
    """hmm.py:792-922.  No boundary condition by default (hmm.py:806-807)."""

    _kind = "elasticity"

    def __init__(self, msh, A, f, msh_micro, eps, petsc_options_global_solve=None, petsc_options_cell_problem=None,
                 petsc_options_prefix: str = "hommx_LinearElasticityHMM", **kw):
        super().__init__(msh, A, f, msh_micro, eps, petsc_options_global_solve, petsc_options_cell_problem,
                         petsc_options_prefix, **kw)

    def _setup_macro_function_space(self):
        return fem.functionspace(self._msh, ("Lagrange", 1, (self._tdim,)))


class LinearElasticityStratifiedHMM(LinearElasticityHMM):
    """hmm.py:925-1067: e_D(u) = sym(Dtheta^T . nabla_grad u) (:1024-1030)."""

    def __init__(self, msh, A, f, msh_micro, eps, Dtheta_transpose, petsc_options_global_solve=None,
                 petsc_options_cell_problem=None, petsc_options_prefix: str = "hommx_LinearElasticityHMM", **kw):
        super().__init__(msh, A, f, msh_micro, eps, petsc_options_global_solve, petsc_options_cell_problem,
                         petsc_options_prefix, **kw)
        self._Dtheta_t = Dtheta_transpose


class PoissonPeriodicHMM:
    """Classical periodic homogenisation, A = A(y) (hmm.py:1070-1279): one cell problem -> constant A_hom -> plain FEM
    macro solve.  ``compute_effective_tensor`` (hmm.py:1219-1245) is a batch of ONE on the GPU."""

    def __init__(self, msh, A, f, msh_micro, eps, petsc_options_global_solve=None, petsc_options_cell_problem=None,
                 petsc_options_prefix: str = "hommx_periodicHMM", **kw):
        self._inner = PoissonHMM(msh, lambda x, y: A(y), f, msh_micro, eps, petsc_options_global_solve,
                                 petsc_options_cell_problem, petsc_options_prefix, **kw)
        self._inner._bcs = []
        self._A_hom = None
        self._correctors = None

    @property
    def function_space(self):
        return self._inner.function_space

    @property
    def A_hom(self):
        return self._A_hom

    def set_boundary_conditions(self, bcs):
        self._inner.set_boundary_conditions(bcs)

    def set_right_hand_side(self, f):
        self._inner.set_right_hand_side(f)

    @property
    def correctors(self) -> list[fem.Function]:
        """One corrector per direction e_q on the micro mesh (hmm.py:1211-1213, filled by compute_effective_tensor :1239-1240)."""
        if self._correctors is None:
            self.compute_effective_tensor()
        return self._correctors

    def compute_effective_tensor(self) -> np.ndarray:
        """hmm.py:1219-1245: one periodic cell problem per direction -> correctors and A_hom (a batch of ONE on the GPU)."""
        h = self._inner
        cells = np.array([0])
        coef, kind = h._element_means(cells)
        AH, chi, info = h._ensure_plan(kind).solve(coef, None, return_info=True, return_correctors=True)
        if info[0]:
            h._logger.error("Something went wrong in the cell problem solving for the periodic cell")
        self._A_hom = AH[0]
        self._correctors = h._on_micro_mesh(chi[0])
        return self._A_hom

    def criterion(self, *args, nonlinear: bool = False, **kw):
        """Not offered here: the nonlinear state belongs to ``PoissonHMM.solve_nonlinear`` (see ``solve_nonlinear``), and the linear
        state of the one periodic cell is ``correctors`` and ``A_hom``."""
        raise RuntimeError("PoissonPeriodicHMM has no criterion(): " + ("the nonlinear state is that of PoissonHMM.solve_nonlinear; " if nonlinear else "")
                           + "use PoissonHMM.criterion")

    def reconstruct(self, *args, nonlinear: bool = False, **kw):
        """Not offered here, as ``criterion``."""
        raise RuntimeError("PoissonPeriodicHMM has no reconstruct(): " + ("the nonlinear state is that of PoissonHMM.solve_nonlinear; " if nonlinear else "")
                           + "use PoissonHMM.reconstruct")

    def solve_nonlinear(self, *args, **kw):
        """Not offered here: with one periodic cell for the whole domain the secant tensor would still differ from macro cell to
        macro cell (it depends on the macro strain), which is what ``PoissonHMM.solve_nonlinear`` computes."""
        raise RuntimeError("PoissonPeriodicHMM has no solve_nonlinear(): the secant tensor depends on the macro strain of every cell; "
                           "use PoissonHMM.solve_nonlinear")

    def solve(self) -> fem.Function:
        """hmm.py:1247-1256: standard P1 FEM with the constant A_hom."""
        if self._A_hom is None:
            self.compute_effective_tensor()
        h = self._inner
        cells = np.arange(h._msh.num_cells)
        S = h._local_stiffness_from_tensors(cells, np.broadcast_to(self._A_hom, (len(cells),) + self._A_hom.shape))
        h._set_macro_matrix(S)
        self._lp_A = h._A
        return h.solve()
