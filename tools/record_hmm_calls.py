"""Record what the solver classes of hommx_amd/hmm.py send to their plan, call by call, and what they return: the fixture
tests/golden/hmm_calls/ (trace.npz + index.json) of tests/test_hmm_call_trace_host.py.

    python tools/record_hmm_calls.py [--tree <checkout of the commit to record>] [--out DIR]

CPU only: a recording stand-in is installed as ``h._plan``.  It uses nothing but the stand-in protocol of ``BaseHMM._coef_stream`` and
public names, so the same file records the parent commit and any later one.  The stand-in answers with deterministic patterns of the
right shapes (no solve: the numbers mean nothing, they only have to be told apart call by call) and appends, for every call, the method,
the keyword names and every argument: an array as itself, a ``CoefStream`` as its method, shared arguments and ``per_cell``, a
``Program`` as its ops, constants and counts.  After a case the public result (every field), ``quadrature_degree_used`` and the
WARNING lines are recorded; a case that raises records the exception's type and text, after the calls made before it.

Cases: seven coefficients on a 4 x 4 macro / 4 x 4 micro square (32 cells of 32 elements) and a 3D elasticity one on 2^3 / 3^3, each
against a stand-in that offers the sampler methods and one that does not, each chunked method once with the default ``chunk_cells`` and
once with 5 (seven chunks, the last one ragged).  Equal arrays are stored once (most chunks recur from method to method).

trace.npz holds the arrays (``a<k>``) and ``cases``, the JSON text of every case with its arrays by key; index.json lists, per case, the
plan methods called in order and the type of the exception, for the reader.
"""

from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PI = 2.0 * np.pi


def pattern(shape, salt: int) -> np.ndarray:
    """Exactly representable numbers in [0, 1.5] that differ from call to call (``salt``) and along every axis."""
    n = int(np.prod(shape))
    return (((np.arange(n) * 7 + 3 * salt) % 13) / 8.0).reshape(shape)


class Store:
    """Arrays by content: equal arrays (shape, dtype, bytes) get one key."""

    def __init__(self):
        self.arrays, self._keys = {}, {}

    def put(self, a) -> dict:
        a = np.ascontiguousarray(a)
        h = hashlib.sha1(repr((a.shape, a.dtype.str)).encode() + a.tobytes()).hexdigest()
        if h not in self._keys:
            self._keys[h] = f"a{len(self._keys)}"
            self.arrays[self._keys[h]] = a
        return {"array": self._keys[h]}


def encode(v, store: Store):
    """A value as JSON: arrays by reference into the store, streams, programs, result dataclasses and functions by their parts."""
    from hommx_amd.batch import CoefStream, Program

    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return {"float": float(v).hex()}
    if isinstance(v, np.ndarray):
        return store.put(v)
    if isinstance(v, CoefStream):
        return {"stream": v.method, "shared": [encode(s, store) for s in v.shared], "per_cell": encode(v.per_cell, store)}
    if isinstance(v, Program):
        return {"program": {f.name: encode(getattr(v, f.name), store) for f in dataclasses.fields(v)}}
    if dataclasses.is_dataclass(v):
        return {type(v).__name__: {f.name: encode(getattr(v, f.name), store) for f in dataclasses.fields(v)}}
    if hasattr(v, "x") and hasattr(v.x, "array"):  # a fem.Function
        return {"function": store.put(v.x.array)}
    if isinstance(v, (tuple, list)):
        return [encode(e, store) for e in v]
    raise TypeError(f"cannot record a {type(v).__name__}")


class RecordingPlan:
    """A stand-in plan without the sampler methods: it gets every coefficient as element means."""

    def __init__(self, dim: int, n: int, kind: str, n_el: int, store: Store):
        self.dim, self.n_micro, self.kind, self.n_el = dim, n, kind, n_el
        self.t = dim if kind.startswith("poisson") else dim * (dim + 1) // 2
        self.bs = 1 if kind.startswith("poisson") else dim
        self.n_nodes = n ** dim
        self.calls, self._store = [], store

    def _note(self, method: str, args: dict, kw: dict) -> int:
        self.calls.append({"method": method, "keywords": sorted(kw), "args": {k: encode(v, self._store) for k, v in {**args, **kw}.items()}})
        return len(self.calls)

    @staticmethod
    def _count(coef) -> int:
        return len(coef)

    def _tensors(self, nc: int, salt: int):
        """Symmetric positive definite A_eff[nc, t, t] and info[nc]."""
        p = pattern((nc, self.t, self.t), salt)
        return 2.0 * np.eye(self.t) + 0.0625 * (p + np.swapaxes(p, 1, 2)), np.zeros(nc, dtype=np.int32)

    def _solved(self, nc, salt, return_info, return_correctors=False):
        A, info = self._tensors(nc, salt)
        if return_correctors:
            corr = pattern((nc, self.t, self.n_nodes * self.bs), salt + 1)
            return (A, corr, info) if return_info else (A, corr)
        return (A, info) if return_info else A

    def reserve(self, n_cells):
        self._note("reserve", {"n_cells": n_cells}, {})

    def solve(self, coef, M=None, **kw):
        salt = self._note("solve", {"coef": coef, "M": M}, kw)
        return self._solved(self._count(coef), salt, kw.get("return_info", False), kw.get("return_correctors", False))

    def reconstruct(self, coef, xi, M=None, **kw):
        from hommx_amd.batch import Reconstruction

        salt, nc, t = self._note("reconstruct", {"coef": coef, "xi": xi, "M": M}, kw), self._count(coef), self.t
        A, info = self._tensors(nc, salt)
        stats = pattern((nc, 2 * t + 3), salt + 1)
        stats[:, 2 * t + 2] = (np.arange(nc) + salt) % self.n_el
        fields = [pattern((nc, self.n_el, t), salt + k) for k in (2, 3)] if kw.get("fields") else [None, None]
        nr = 0 if kw.get("regions") is None else (kw.get("n_regions") or 2)
        rs = None
        if nr:
            rs = pattern((nc, nr, 2 * t + 4), salt + 4) + 0.125
            rs[:, :, 2 * t + 3] = (np.arange(nc)[:, None] + np.arange(nr)[None, :] + salt) % self.n_el
        return Reconstruction.from_stats(np.asarray(xi), stats, A, info, *fields, region_stats=rs)

    def loads(self, coef, P, M=None, **kw):
        from hommx_amd.batch import LoadResponse

        salt, nc, t = self._note("loads", {"coef": coef, "P": P, "M": M}, kw), self._count(coef), self.t
        nl = P.shape[1] if kw.get("per_cell") else P.shape[0]
        A, info = self._tensors(nc, salt)
        r = LoadResponse(pattern((nc, nl, t), salt + 1), A, info)
        if kw.get("response") or kw.get("fields") or kw.get("return_correctors"):
            r.energy, r.mean_flux, r.max_flux = pattern((nc, nl, nl), salt + 2), pattern((nc, nl, t), salt + 3), pattern((nc, nl), salt + 4)
            r.argmax_element = ((np.arange(nc * nl) + salt) % self.n_el).reshape(nc, nl).astype(np.int64)
        if kw.get("fields"):
            r.strain, r.flux = pattern((nc, nl, self.n_el, t), salt + 5), pattern((nc, nl, self.n_el, t), salt + 6)
        if kw.get("return_correctors"):
            r.correctors = pattern((nc, nl, self.n_nodes * self.bs), salt + 7)
        return r

    def _n_dirs(self, coef, directions, per_cell) -> int:
        if isinstance(directions, str):
            prog = coef.shared[2]
            return prog.n_params + prog.n_fields
        return directions.shape[1] if per_cell else directions.shape[0]

    def sensitivities(self, coef, M=None, **kw):
        from hommx_amd.batch import Sensitivities

        salt, nc, t = self._note("sensitivities", {"coef": coef, "M": M}, kw), self._count(coef), self.t
        nd = self._n_dirs(coef, kw.get("directions"), kw.get("per_cell"))
        return Sensitivities(pattern((nc, nd, t, t), salt + 1), None, *self._tensors(nc, salt))

    def second_sensitivities(self, coef, M=None, **kw):
        from hommx_amd.batch import SecondSensitivities

        salt, nc, t = self._note("second_sensitivities", {"coef": coef, "M": M}, kw), self._count(coef), self.t
        nd = self._n_dirs(coef, kw.get("directions"), kw.get("per_cell"))
        return SecondSensitivities(pattern((nc, nd, nd, t, t), salt + 1), pattern((nc, nd, t, t), salt + 2) if kw.get("first") else None,
                                   *self._tensors(nc, salt))

    def stratification_sensitivities(self, coef, M=None, **kw):
        from hommx_amd.batch import StratSensitivities

        salt, nc, t, d = self._note("stratification_sensitivities", {"coef": coef, "M": M}, kw), self._count(coef), self.t, self.dim
        return StratSensitivities(pattern((nc, d, d, t, t), salt + 1) if kw.get("full", True) else None,
                                  None if kw.get("weights") is None else pattern((nc, d, d), salt + 2), *self._tensors(nc, salt))


class SamplerRecordingPlan(RecordingPlan):
    """A stand-in that offers the three sampler methods: it gets ``TwoPhase``, ``Separable`` and ``Expression`` as their streams."""

    def solve_two_phase(self, mask, values, M=None, **kw):
        salt = self._note("solve_two_phase", {"mask": mask, "values": values, "M": M}, kw)
        return self._solved(len(values), salt, kw.get("return_info", False))

    def solve_separable(self, family, table, weights, params, M=None, **kw):
        salt = self._note("solve_separable", {"family": family, "table": table, "weights": weights, "params": params, "M": M}, kw)
        return self._solved(len(params), salt, kw.get("return_info", False))

    def solve_program(self, points, weights, program, midpoints, M=None, **kw):
        salt = self._note("solve_program", {"points": points, "weights": weights, "program": program, "midpoints": midpoints, "M": M}, kw)
        return self._solved(len(midpoints), salt, kw.get("return_info", False))


# -- the solvers ------------------------------------------------------------------------------------------------------------------------------
def _stripe(y):
    return (y[0] > 0.25) & (y[0] < 0.75)


def _dtheta(x):
    """A non-constant Dtheta_transpose that broadcasts over cells."""
    one = 1.0 + 0.0 * x[0]
    return [[one + 0.25 * x[1], 0.5 * x[0]], [0.0 * one, one - 0.125 * x[0]]]


def _dtheta_dphi(x):
    one = 1.0 + 0.0 * x[0]
    return [[0.0 * one, one], [-one, 0.25 * x[1]]]


def solvers() -> dict:
    """name -> constructor of the solver of one coefficient."""
    from hommx_amd import hmm, mesh
    from hommx_amd.expr import Expression

    sq = lambda: (mesh.create_unit_square(4, 4), mesh.create_unit_square(4, 4))
    rhs = lambda x: 1.0 + x[0]
    lame = lambda lam, mu: (lambda x: hmm.Lame(lam + 0.5 * x[0], mu + 0.25 * x[1]))

    def expression(text="2 + p[0]*x[0] + p[1]*sin(2*pi*y[0]) + f[0]*y[1]"):
        msh, mic = sq()
        h = hmm.PoissonHMM(msh, Expression(text, p=[0.5, 0.25], parameter_names=("slope", "wave"), fields=("design",)), rhs, mic, 0.01)
        h.set_fields(0.125 + 0.5 * msh.cell_midpoints()[:, 1])
        return h

    def elastic(msh, mic, A):
        h = hmm.LinearElasticityHMM(msh, A, lambda x: np.array([0.0, -1.0, 0.0][: msh.topology.dim]), mic, 0.01)
        h.set_boundary_conditions(hmm.fem.dirichletbc(np.zeros(msh.topology.dim), hmm._box_boundary_nodes(msh), h.function_space))
        return h

    return {
        "callable": lambda: hmm.PoissonHMM(*sq()[:1], lambda x, y: 2.0 + x[0] + np.sin(TWO_PI * y[0]) * np.cos(TWO_PI * y[1]), rhs, sq()[1], 0.01,
                                           quadrature_degree=0),
        "two_phase": lambda: hmm.PoissonHMM(*sq()[:1], hmm.TwoPhase(_stripe, lambda x: 5.0 + 2.0 * x[0], lambda x: 1.0 + 0.5 * x[1]), rhs, sq()[1], 0.01),
        "affine": lambda: hmm.PoissonHMM(*sq()[:1], hmm.Separable("affine", lambda x: 1.5 + x[0], lambda x: 0.25 + 0.125 * x[1],
                                                                   lambda y: np.sin(TWO_PI * y[0])), rhs, sq()[1], 0.01),
        "reciprocal": lambda: hmm.PoissonHMM(*sq()[:1], hmm.Separable("reciprocal", lambda x: 2.0 + x[0], lambda x: 0.5 + 0.0 * x[0],
                                                                       lambda y: np.cos(TWO_PI * y[0])), rhs, sq()[1], 0.01),
        "expression": expression,
        "expression_curved": lambda: expression("2 + p[0]*p[1]*x[0] + tanh(f[0]*y[1])"),
        "lame": lambda: elastic(*sq(), hmm.TwoPhase(_stripe, lame(4.0, 3.0), lame(1.0, 1.5))),
        "stratified": lambda: hmm.PoissonStratifiedHMM(*sq()[:1], lambda x, y: 1.5 + 0.5 * x[1] + 0.25 * np.sin(TWO_PI * (y[0] + y[1])), rhs, sq()[1], 0.01,
                                                       _dtheta, quadrature_degree=3),
        "lame3d": lambda: elastic(mesh.create_unit_cube(2, 2, 2), mesh.create_unit_cube(3, 3, 3),
                                  hmm.TwoPhase(lambda y: y[2] > 0.5, lame(4.0, 3.0), lame(1.0, 1.5))),
    }


def macro_field(h, k: int = 0) -> np.ndarray:
    """A smooth dof vector of the macro space (``k``: another one)."""
    x = h._msh.geometry.x
    f = np.sin(2.0 * x[:, 0] + k) + x[:, 1] ** 2 * (1 + k)
    return f if h._bs == 1 else np.stack([f * (1.0 + 0.5 * c) + 0.25 * c * x[:, 0] for c in range(h._bs)], axis=1).ravel()


def _polarisation_callable(h):
    t = h._tensor_size()
    return lambda x, y: [0.5 * (c + 1) + x[0] * np.sin(TWO_PI * y[0]) for c in range(t)]


def _with_polarisation(kind):
    def prepare(h):
        n_el, t = h._cell_mesh.num_cells, h._tensor_size()
        h.set_polarisation({"shared": lambda: pattern((n_el, t), 5), "per_cell": lambda: pattern((h._msh.num_cells, n_el, t), 6),
                            "callable": lambda: _polarisation_callable(h)}[kind]())
    return prepare


def _direction_a(x, y):
    return 1.0 + 0.0 * x[0] + np.sin(TWO_PI * y[1])


def _direction_b(x, y):
    return x[0] * np.cos(TWO_PI * y[0])


def _lame_direction(x, y):
    from hommx_amd.hmm import Lame

    return Lame(1.0 + 0.0 * x[0] + 0.0 * y[0], x[1] + np.sin(TWO_PI * y[0]))


def methods(name: str) -> list:
    """(case name, takes chunk_cells, prepare(h) or None, run(h, **chunk)) of the solver ``name``."""
    dirs = [_lame_direction] if name.startswith("lame") else [_direction_a, _direction_b]
    with_parameters = name in ("two_phase", "affine", "expression", "expression_curved", "lame", "lame3d")
    expr = name.startswith("expression")
    out = [
        ("solve", False, None, lambda h: h.solve()),
        ("reconstruct", True, None, lambda h, **c: h.reconstruct(macro_field(h), **c)),
        ("tensor_derivatives_directions", True, None, lambda h, **c: h.tensor_derivatives(directions=dirs, **c)),
    ]
    if name == "lame3d":  # the 3D case: the paths whose shapes depend on the dimension
        return out + [("tensor_derivatives", True, None, lambda h, **c: h.tensor_derivatives(**c))]
    some = np.array([30, 2, 17, 9, 11, 4, 25])
    out += [
        ("solve_polarisation_array", False, _with_polarisation("shared"), lambda h: (h.solve(), h.effective_polarisation)),
        ("solve_polarisation_per_cell", False, _with_polarisation("per_cell"), lambda h: (h.solve(), h.effective_polarisation)),
        ("solve_polarisation_callable", False, _with_polarisation("callable"), lambda h: (h.solve(), h.effective_polarisation)),
        ("solve_then_reconstruct", True, None, lambda h, **c: (h.solve(), h.reconstruct(**c), h.cell_means())),
        ("reconstruct_fields", True, None, lambda h, **c: h.reconstruct(macro_field(h), cells=some, fields=True, **c)),
        ("reconstruct_callable_regions", True, None,
         lambda h, **c: h.reconstruct(macro_field(h), regions=lambda y: (3 * y[0]).astype(int) + 3 * (y[1] > 0.5), **c)),
        ("load_response", True, _with_polarisation("callable"), lambda h, **c: h.load_response(**c)),
        ("load_response_fields", True, _with_polarisation("shared"), lambda h, **c: h.load_response(cells=some, fields=True, correctors=True, **c)),
        ("tensor_second_derivatives_directions", True, None, lambda h, **c: h.tensor_second_derivatives(directions=dirs, **c)),
        ("energy_derivatives", True, None, lambda h, **c: h.energy_derivatives(macro_field(h), macro_field(h, 1), directions=dirs, **c)),
        ("energy_second_derivatives", True, None, lambda h, **c: h.energy_second_derivatives(macro_field(h), directions=dirs, cells=some, **c)),
        ("stratification_derivatives", True, None, lambda h, **c: h.stratification_derivatives(**c)),
        ("stratification_derivatives_parameters", True, None, lambda h, **c: h.stratification_derivatives(cells=some, parameters=[_dtheta_dphi], **c)),
        ("stratification_energy_derivatives", False, None, lambda h: h.stratification_energy_derivatives(macro_field(h), macro_field(h, 1))),
        ("stratification_energy_derivatives_parameters", False, None,
         lambda h: (h.solve(), h.stratification_energy_derivatives(cells=some, parameters=[_dtheta_dphi, _dtheta]))[1]),
        ("cell_means", False, None, lambda h: h.cell_means(macro_field(h))),
        ("correctors_for_cell", False, None, lambda h: h.correctors_for_cell(7)),
        ("prepare", False, None, lambda h: h.prepare() is h),
        # refusals
        ("refuse_reconstruct_unsolved", False, None, lambda h: h.reconstruct()),
        ("refuse_reconstruct_dofs", False, None, lambda h: h.reconstruct(np.zeros(3))),
        ("refuse_reconstruct_empty", False, None, lambda h: h.reconstruct(macro_field(h), cells=[])),
        ("refuse_cell_means_unsolved", False, None, lambda h: h.cell_means()),
        ("refuse_cell_means_dofs", False, None, lambda h: h.cell_means(np.zeros(3))),
        ("refuse_load_response_none", False, None, lambda h: h.load_response()),
        ("refuse_load_response_empty", False, _with_polarisation("shared"), lambda h: h.load_response(cells=[])),
        ("refuse_tensor_derivatives_empty", False, None, lambda h: h.tensor_derivatives(cells=[])),
        ("refuse_tensor_second_derivatives_empty", False, None, lambda h: h.tensor_second_derivatives(cells=np.zeros((0, 2)))),
        ("refuse_energy_derivatives_unsolved", False, None, lambda h: h.energy_derivatives(directions=dirs)),
        ("refuse_energy_derivatives_dofs", False, None, lambda h: h.energy_derivatives(macro_field(h), np.zeros(2), directions=dirs)),
        ("refuse_energy_second_derivatives_unsolved", False, None, lambda h: h.energy_second_derivatives(directions=dirs)),
        ("refuse_stratification_derivatives_empty", False, None, lambda h: h.stratification_derivatives(cells=[])),
        ("refuse_stratification_parameters_empty", False, None, lambda h: h.stratification_derivatives(parameters=[])),
        ("refuse_stratification_energy_unsolved", False, None, lambda h: h.stratification_energy_derivatives()),
        ("refuse_stratification_energy_empty", False, None, lambda h: h.stratification_energy_derivatives(macro_field(h), cells=[])),
        ("refuse_stratification_energy_dofs", False, None, lambda h: h.stratification_energy_derivatives(np.zeros(4))),
        ("refuse_curvature_directions", False, None, lambda h: h.tensor_second_derivatives(directions=dirs, curvature=True)),
        ("refuse_direction_shape", False, None, lambda h: h.tensor_derivatives(directions=[_direction_a if dirs[0] is _lame_direction else _lame_direction])),
        # without directions: the parameters of the coefficient, or the refusal that names what has them
        ("tensor_derivatives", True, None, lambda h, **c: h.tensor_derivatives(**c)),
        ("tensor_second_derivatives", True, None, lambda h, **c: h.tensor_second_derivatives(**c)),
        ("tensor_second_derivatives_curvature", True, None, lambda h, **c: h.tensor_second_derivatives(curvature=True, **c)),
    ]
    if with_parameters:
        out.append(("energy_derivatives_parameters", True, None, lambda h, **c: h.energy_derivatives(macro_field(h), cells=some, **c)))
    if name in ("two_phase", "lame"):
        out.append(("reconstruct_regions", True, None, lambda h, **c: h.reconstruct(macro_field(h), regions=True, **c)))
    else:
        out.append(("refuse_regions_true", False, None, lambda h: h.reconstruct(macro_field(h), regions=True)))
    if expr:
        def unset(h):
            h._fields = None

        def no_slots(h):
            from hommx_amd.expr import Expression

            h._coeff = Expression("2 + x[0] + sin(2*pi*y[0])")

        out += [("refuse_fields_unset", False, unset, lambda h: h.tensor_derivatives()),
                ("refuse_fields_unset_curvature", False, unset, lambda h: h.tensor_second_derivatives(curvature=True, directions=dirs)),
                ("refuse_curvature_no_slots", False, no_slots, lambda h: h.tensor_second_derivatives(curvature=True)),
                ("set_parameters", True, lambda h: h.set_parameters([0.75, 0.5]), lambda h, **c: h.tensor_derivatives(**c))]
    return out


def periodic_case(plan_cls, store: Store) -> dict:
    """``PoissonPeriodicHMM.solve`` (and its correctors) on the 4 x 4 squares."""
    from hommx_amd import hmm, mesh

    per = hmm.PoissonPeriodicHMM(mesh.create_unit_square(4, 4), lambda y: 2.0 + np.sin(TWO_PI * y[0]), lambda x: 1.0 + x[0],
                                 mesh.create_unit_square(4, 4), 0.01, quadrature_degree=3)
    per.set_boundary_conditions(hmm.fem.dirichletbc(0.0, hmm._box_boundary_nodes(per._inner._msh), per.function_space))
    return run_case(per._inner, plan_cls, store, lambda h: (per.solve(), per.A_hom, per.correctors))


class _Warnings(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def run_case(h, plan_cls, store: Store, run, prepare=None, **chunk) -> dict:
    plan = plan_cls(h._tdim, h._n_micro, "poisson" if h._kind == "poisson" else "elasticity", h._cell_mesh.num_cells, store)
    h._plan = plan
    log, seen = logging.getLogger("hommx_amd.hmm"), _Warnings()
    log.addHandler(seen)
    case = {}
    try:
        if prepare is not None:
            prepare(h)
        case["result"] = encode(run(h, **chunk), store)
    except Exception as exc:  # a refusal: what was raised, after what had been sent
        case["raises"] = [type(exc).__name__, str(exc)]
    finally:
        log.removeHandler(seen)
    case.update(calls=plan.calls, quadrature_degree_used=h.quadrature_degree_used, warnings=seen.lines)
    return case


def record() -> tuple[dict, dict]:
    """(index, arrays): every case by name, and the arrays the index refers to."""
    store, index = Store(), {}
    for plan_cls in (RecordingPlan, SamplerRecordingPlan):
        tag = "sampler" if plan_cls is SamplerRecordingPlan else "means"
        for name, make in solvers().items():
            for case, chunked, prepare, run in methods(name):
                if case.startswith("stratification") and not case.startswith("stratification_energy") and name not in ("stratified", "two_phase", "lame"):
                    continue  # the M = I branch is the same for every other coefficient
                for chunk in ({}, {"chunk_cells": 5}) if chunked else ({},):
                    index[f"{tag}/{name}/{case}" + ("/chunk5" if chunk else "")] = run_case(make(), plan_cls, store, run, prepare, **chunk)
        index[f"{tag}/periodic/solve"] = periodic_case(plan_cls, store)
    return index, store.arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="the checkout whose hommx_amd is recorded")
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "hmm_calls"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    cases, arrays = record()
    os.makedirs(a.out, exist_ok=True)
    text = json.dumps(cases, separators=(",", ":"), sort_keys=True).encode()
    np.savez_compressed(os.path.join(a.out, "trace.npz"), cases=np.frombuffer(text, dtype=np.uint8), **arrays)
    with open(os.path.join(a.out, "index.json"), "w") as f:  # for the reader: what is in the trace
        json.dump({name: {"calls": [c["method"] for c in case["calls"]], "raises": case.get("raises", [None])[0]} for name, case in cases.items()},
                  f, indent=0, sort_keys=True)
        f.write("\n")
    raised = sum("raises" in c for c in cases.values())
    print(f"{len(cases)} cases ({raised} refusals), {sum(len(c['calls']) for c in cases.values())} calls, {len(arrays)} arrays")


def load(folder: str) -> tuple[dict, dict]:
    """(cases, arrays) of a recorded trace."""
    with np.load(os.path.join(folder, "trace.npz")) as z:
        arrays = {k: z[k] for k in z.files if k != "cases"}
        return json.loads(z["cases"].tobytes().decode()), arrays


if __name__ == "__main__":
    main()
