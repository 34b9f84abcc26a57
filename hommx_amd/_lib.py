"""ctypes binding of libhommx_hip.so (include/hommx_hip.h).

The library is the product path; there is NO CPU fallback.  If the shared object is missing or
cannot be loaded, every entry point raises -- loudly -- instead of computing something else.
"""

from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HOMMX_LIB") or os.path.join(_HERE, "libhommx_hip.so")  # HOMMX_LIB: A/B builds (dev)

KIND_POISSON_SCALAR = 0
KIND_POISSON_MATRIX = 1
KIND_ELASTICITY_ISO = 2
KIND_ELASTICITY_VOIGT = 3
SAMPLER_AFFINE = 0
SAMPLER_RECIPROCAL = 1
MESH_MAX_FRONT = 192  # HOMMX_MESH_MAX_FRONT
MESH_FLAG_TREE = 1  # HOMMX_MESH_FLAG_TREE
MESH_FLAG_LOADS = 2  # HOMMX_MESH_FLAG_LOADS
FLAG_TREE_LOADS = 4  # HOMMX_FLAG_TREE_LOADS == HOMMX_MESH_FLAG_TREE_LOADS: load solves of a tree plan substitute on its kept fronts
COEF_SAMPLED = 0  # HOMMX_COEF_*: the form of a hommx_coef_source
COEF_TWO_PHASE = 1
COEF_SEPARABLE = 2
COEF_PROGRAM = 3
PROGRAM_MAX_OPS, PROGRAM_MAX_CONSTS, PROGRAM_MAX_STACK = 128, 32, 16  # the limits of a hommx_coef_program
RECON_MAX_REGIONS = 8  # HOMMX_RECON_MAX_REGIONS
SENS_MAX_DIRS = 8  # HOMMX_SENS_MAX_DIRS
PROGRAM_MAX_PARAMS = 4  # HOMMX_PROGRAM_MAX_PARAMS
PROGRAM_MAX_FIELDS = 4  # HOMMX_PROGRAM_MAX_FIELDS
DIRS_PARAMETERS = 2  # HOMMX_DIRS_PARAMETERS: per_cell of SensArgs / Sens2Args, the directions are the program's parameter tangents
DIRS_PARAMETERS_CURVATURE = 3  # HOMMX_DIRS_PARAMETERS_CURVATURE: per_cell of Sens2Args, d2A takes the curvature term as well (the Hessian)
LOADS_SHARED, LOADS_PER_CELL, LOADS_PROGRAM = 0, 1, 2  # HOMMX_LOADS_*: per_cell of LoadArgs, where the load comes from
LOADS_EIGENSTRAIN = 4  # HOMMX_LOADS_EIGENSTRAIN: a flag or-ed to them, what arrives is an eigenstrain
CRIT_NSTATS = 4  # HOMMX_CRIT_NSTATS: max, argmax element, sum |K| v, sum |K| [v >= threshold]
SECANT_NSTATE = 3  # HOMMX_SECANT_NSTATE: rounds, change, status
SECANT_MAX_HISTORY = 4  # HOMMX_SECANT_MAX_HISTORY: the history variables of a law


class PlanDesc(C.Structure):
    _fields_ = [
        ("dim", C.c_int32),
        ("n_micro", C.c_int32),
        ("kind", C.c_int32),
        ("device", C.c_int32),
        ("flags", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class MeshDesc(C.Structure):
    _fields_ = [
        ("dim", C.c_int32),
        ("kind", C.c_int32),
        ("device", C.c_int32),
        ("flags", C.c_int32),
        ("n_nodes", C.c_int64),
        ("n_el", C.c_int64),
        ("el_nodes", C.c_void_p),
        ("el_x", C.c_void_p),
        ("order", C.c_void_p),
        ("reserved", C.c_int32 * 4),
    ]


class CoefProgram(C.Structure):
    """hommx_coef_program: the postfix program of an expression coefficient (host memory, also in the device entries)."""

    _fields_ = [
        ("n_ops", C.c_int32),
        ("n_consts", C.c_int32),
        ("n_comp", C.c_int32),
        ("n_params", C.c_int32),  # the first n_params constants are the parameters (0 .. PROGRAM_MAX_PARAMS)
        ("ops", C.c_void_p),
        ("consts", C.c_void_p),
    ]


class _SourceFields(C.Union):
    """The member of hommx_coef_source that was ``reserved`` (0) and is ``n_fields`` now: both names, one word."""

    _fields_ = [("n_fields", C.c_int32), ("reserved", C.c_int32)]


class CoefSource(C.Structure):
    """hommx_coef_source: only the pointers of ``form`` are read; ``n_fields`` (HOMMX_COEF_PROGRAM: fields per macro cell after the
    midpoint in ``params``, 0 .. PROGRAM_MAX_FIELDS) for that form only."""

    _anonymous_ = ("_fields_word",)
    _fields_ = [
        ("form", C.c_int32),
        ("family", C.c_int32),
        ("n_q", C.c_int32),
        ("_fields_word", _SourceFields),
        ("coef", C.c_void_p),
        ("mask", C.c_void_p),
        ("values", C.c_void_p),
        ("table", C.c_void_p),
        ("weights", C.c_void_p),
        ("params", C.c_void_p),
        ("program", C.POINTER(CoefProgram)),
    ]


class SensArgs(C.Structure):
    """hommx_sens_args: what hommx_sensitivity_source[_device] is asked for and where it goes."""

    _fields_ = [
        ("n_dirs", C.c_int32),
        ("per_cell", C.c_int32),
        ("dirs", C.c_void_p),
        ("dA", C.c_void_p),
        ("weights", C.c_void_p),
        ("grad", C.c_void_p),
        ("A_eff", C.c_void_p),
        ("info", C.c_void_p),
    ]


class Sens2Args(C.Structure):
    """hommx_sens2_args: what hommx_second_sensitivity_source[_device] is asked for and where it goes."""

    _fields_ = [
        ("n_dirs", C.c_int32),
        ("per_cell", C.c_int32),
        ("dirs", C.c_void_p),
        ("d2A", C.c_void_p),
        ("dA", C.c_void_p),
        ("A_eff", C.c_void_p),
        ("info", C.c_void_p),
    ]


class StratSensArgs(C.Structure):
    """hommx_strat_sens_args: what hommx_stratification_sensitivity_source[_device] is asked for and where it goes."""

    _fields_ = [
        ("dA_dM", C.c_void_p),
        ("weights", C.c_void_p),
        ("grad_M", C.c_void_p),
        ("A_eff", C.c_void_p),
        ("info", C.c_void_p),
    ]


class LoadArgs(C.Structure):
    """hommx_load_args: the loads of hommx_loads_source[_device], what is asked for and where it goes.  ``P_source`` is read for
    ``LOADS_PROGRAM`` only."""

    _fields_ = [
        ("n_loads", C.c_int32),
        ("per_cell", C.c_int32),
        ("P", C.c_void_p),
        ("P_eff", C.c_void_p),
        ("A_eff", C.c_void_p),
        ("energy", C.c_void_p),
        ("stats", C.c_void_p),
        ("strain", C.c_void_p),
        ("flux", C.c_void_p),
        ("correctors", C.c_void_p),
        ("info", C.c_void_p),
        ("P_source", C.POINTER(CoefSource)),
    ]


class CriterionArgs(C.Structure):
    """hommx_criterion_args: the criterion of hommx_criterion_source[_device], its one optional load, what is asked for and where it
    goes.  The load members are read with ``has_load`` only, ``P_source`` for ``LOADS_PROGRAM`` only."""

    _fields_ = [
        ("program", C.POINTER(CoefProgram)),
        ("n_fields", C.c_int32),
        ("rows", C.c_void_p),
        ("points", C.c_void_p),
        ("xi", C.c_void_p),
        ("threshold", C.c_double),
        ("has_load", C.c_int32),
        ("per_cell", C.c_int32),
        ("P", C.c_void_p),
        ("P_source", C.POINTER(CoefSource)),
        ("crit", C.c_void_p),
        ("values", C.c_void_p),
        ("strain", C.c_void_p),
        ("flux", C.c_void_p),
        ("A_eff", C.c_void_p),
        ("info", C.c_void_p),
    ]


class SecantArgs(C.Structure):
    """hommx_secant_args: the law of hommx_secant_source[_device], the iteration's limits, an optional start stream and where the
    outputs of every cell's stopping round go."""

    _fields_ = [
        ("program", C.POINTER(CoefProgram)),
        ("n_fields", C.c_int32),
        ("rows", C.c_void_p),
        ("points", C.c_void_p),
        ("xi", C.c_void_p),
        ("max_iter", C.c_int32),
        ("tol", C.c_double),
        ("relax", C.c_double),
        ("coef_start", C.c_void_p),
        ("state", C.c_void_p),
        ("A_eff", C.c_void_p),
        ("mean_flux", C.c_void_p),
        ("coef_out", C.c_void_p),
        ("strain", C.c_void_p),
        ("flux", C.c_void_p),
        ("law_values", C.c_void_p),
        ("info", C.c_void_p),
    ]


class SecantTangentArgs(C.Structure):
    """hommx_secant_tangent_args: the iteration (a SecantArgs), the sibling plan of the tangent kind and where D, the asymmetry, the
    tangent stream and the info of the tangent elimination go."""

    _fields_ = [
        ("secant", C.POINTER(SecantArgs)),
        ("tangent_plan", C.c_void_p),
        ("tangent", C.c_void_p),
        ("asymmetry", C.c_void_p),
        ("tangent_coef", C.c_void_p),
        ("tangent_info", C.c_void_p),
    ]


class HistoryArgs(C.Structure):
    """hommx_history_args: the history variables of a law -- their number, the history at the start of the call and where the updates
    of every cell's stopping round go."""

    _fields_ = [
        ("n_history", C.c_int32),
        ("history_in", C.c_void_p),
        ("history_out", C.c_void_p),
    ]


class SecantLoadArgs(C.Structure):
    """hommx_secant_load_args: the one load beside a law -- its code (LOADS_PER_CELL or LOADS_PROGRAM, alone or with
    LOADS_EIGENSTRAIN), the per-cell array or the program source."""

    _fields_ = [
        ("per_cell", C.c_int32),
        ("P", C.c_void_p),
        ("P_source", C.POINTER(CoefSource)),
    ]


class SecantStateArgs(C.Structure):
    """hommx_secant_state_args: the tail behind the secant iteration on the state it stopped in -- a criterion (its program on the
    row ``[.. | c | h | b]``, its own fields and rows, the threshold and where its outputs go) and / or the reconstruction statistics."""

    _fields_ = [
        ("crit_program", C.POINTER(CoefProgram)),
        ("crit_n_fields", C.c_int32),
        ("crit_rows", C.c_void_p),
        ("threshold", C.c_double),
        ("crit", C.c_void_p),
        ("crit_values", C.c_void_p),
        ("total_strain", C.c_void_p),
        ("total_flux", C.c_void_p),
        ("reconstruct", C.c_int32),
        ("n_regions", C.c_int32),
        ("region", C.c_void_p),
        ("stats", C.c_void_p),
        ("region_stats", C.c_void_p),
    ]


def _prototypes() -> dict:
    """name -> (restype, argtypes) of every symbol include/hommx_hip.h declares: ``load()`` declares them from this table, and
    the tests check that the header and the library export exactly these names."""
    c_int, f64, char_p = C.c_int, C.c_double, C.c_char_p
    vp, i32, i64, dp = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
    vpp, i32p, i64p = C.POINTER(vp), C.POINTER(i32), C.POINTER(i64)
    return {
        "hommx_device_count": (c_int, []),
        "hommx_plan_create": (c_int, [vpp, C.POINTER(PlanDesc)]),
        "hommx_plan_destroy": (c_int, [vp]),
        "hommx_plan_reserve": (c_int, [vp, i64]),
        "hommx_plan_dim": (i32, [vp]),
        "hommx_plan_device": (i32, [vp]),
        "hommx_plan_n_micro": (i32, [vp]),
        "hommx_plan_kind": (i32, [vp]),
        "hommx_plan_num_elements": (i64, [vp]),
        "hommx_plan_coef_components": (i32, [vp]),
        "hommx_plan_tensor_size": (i32, [vp]),
        "hommx_plan_kernel_name": (char_p, [vp]),
        "hommx_plan_corrector_kernel_name": (char_p, [vp]),
        "hommx_plan_load_kernel_name": (char_p, [vp]),
        "hommx_plan_route_detail": (char_p, [vp]),
        "hommx_plan_flops_per_solve": (f64, [vp]),
        "hommx_mesh_analyze": (c_int, [C.POINTER(MeshDesc), i32p, dp]),
        "hommx_mesh_analyze_tree": (c_int, [C.POINTER(MeshDesc), i32p, i32p, i32p, dp, vp, vp]),
        "hommx_plan_create_mesh": (c_int, [vpp, C.POINTER(MeshDesc)]),
        "hommx_plan_front_width": (i32, [vp]),
        "hommx_solve_batch": (c_int, [vp, i64, vp, vp, vp, vp]),
        "hommx_solve_batch_device": (c_int, [vp, i64, vp, vp, vp, vp, vp]),
        "hommx_solve_batch_correctors": (c_int, [vp, i64, vp, vp, vp, vp, vp]),
        "hommx_solve_batch_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp, vp]),
        "hommx_solve_batch_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp, vp, vp]),
        "hommx_expand_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp]),
        "hommx_expand_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp]),
        "hommx_expand_tangents": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp]),
        "hommx_expand_tangents_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp, vp]),
        "hommx_expand_second_tangents": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp, vp]),
        "hommx_expand_second_tangents_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp, vp, vp]),
        "hommx_reconstruct_batch": (c_int, [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "hommx_reconstruct_batch_device": (c_int, [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "hommx_reconstruct_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "hommx_reconstruct_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "hommx_sensitivity_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SensArgs)]),
        "hommx_sensitivity_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SensArgs), vp]),
        "hommx_second_sensitivity_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(Sens2Args)]),
        "hommx_second_sensitivity_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(Sens2Args), vp]),
        "hommx_stratification_sensitivity_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(StratSensArgs)]),
        "hommx_stratification_sensitivity_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(StratSensArgs), vp]),
        "hommx_loads_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(LoadArgs)]),
        "hommx_loads_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(LoadArgs), vp]),
        "hommx_criterion_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(CriterionArgs)]),
        "hommx_criterion_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(CriterionArgs), vp]),
        "hommx_secant_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs)]),
        "hommx_secant_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs), vp]),
        "hommx_secant_tangent_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantTangentArgs)]),
        "hommx_secant_tangent_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantTangentArgs), vp]),
        "hommx_secant_history_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs), C.POINTER(HistoryArgs)]),
        "hommx_secant_history_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs), C.POINTER(HistoryArgs), vp]),
        "hommx_secant_tangent_history_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantTangentArgs),
                                                        C.POINTER(HistoryArgs)]),
        "hommx_secant_tangent_history_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantTangentArgs),
                                                               C.POINTER(HistoryArgs), vp]),
        "hommx_secant_load_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs), C.POINTER(HistoryArgs),
                                             C.POINTER(SecantLoadArgs)]),
        "hommx_secant_load_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs), C.POINTER(HistoryArgs),
                                                    C.POINTER(SecantLoadArgs), vp]),
        "hommx_secant_state_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs), C.POINTER(HistoryArgs),
                                              C.POINTER(SecantLoadArgs), C.POINTER(SecantStateArgs)]),
        "hommx_secant_state_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantArgs), C.POINTER(HistoryArgs),
                                                     C.POINTER(SecantLoadArgs), C.POINTER(SecantStateArgs), vp]),
        "hommx_secant_tangent_load_source": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantTangentArgs),
                                                     C.POINTER(HistoryArgs), C.POINTER(SecantLoadArgs)]),
        "hommx_secant_tangent_load_source_device": (c_int, [vp, i64, C.POINTER(CoefSource), vp, C.POINTER(SecantTangentArgs),
                                                            C.POINTER(HistoryArgs), C.POINTER(SecantLoadArgs), vp]),
        "hommx_solve_batch_two_phase": (c_int, [vp, i64, vp, vp, vp, vp, vp]),
        "hommx_solve_batch_two_phase_device": (c_int, [vp, i64, vp, vp, vp, vp, vp, vp]),
        "hommx_solve_batch_separable": (c_int, [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp]),
        "hommx_solve_batch_separable_device": (c_int, [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "hommx_comm_init_all": (c_int, [vpp, c_int, C.POINTER(c_int)]),
        "hommx_comm_destroy": (c_int, [vp]),
        "hommx_comm_size": (c_int, [vp]),
        "hommx_allgather_field": (c_int, [vp, vpp, i64]),
        "hommx_solve_batch_multi": (c_int, [vp, vpp, i64, vp, vp, vp, vp]),
        "hommx_solve_batch_multi_device": (c_int, [vp, vpp, i64, vpp, vpp, vpp]),
        "hommx_shard_range": (c_int, [i64, i32, i32, i64p, i64p, i64p]),
        "hommx_unpack_field": (c_int, [i64, i32, i32, vp, vp, vp]),
        "hommx_calibrate_fp64": (c_int, [c_int, dp, dp]),
        "hommx_calibrate_fp64_mfma": (c_int, [c_int, dp]),
        "hommx_calibrate_fp64_detail": (c_int, [c_int, dp, dp, dp]),
        "hommx_last_error": (char_p, []),
    }


PROTOTYPES = _prototypes()
EXPORTED_SYMBOLS = tuple(PROTOTYPES)


class HommxLibraryError(RuntimeError):
    pass


_lib = None


def _share_hip_runtime_with_torch():
    """One process, one HIP runtime.  PyTorch-ROCm wheels bundle their own ``libamdhip64.so.7``; libhommx_hip.so needs the
    same SONAME.  Whichever copy is loaded first serves both, and torch cannot find a GPU when that is not its own copy
    ("No HIP GPUs are available" if libhommx_hip.so was loaded before ``import torch``).  So when torch is installed but not
    imported yet, its copy is loaded first, by path (no ``import torch``: the product does not depend on it)."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:  # pragma: no cover - fall back to the system runtime
            pass


def load():
    """Load libhommx_hip.so (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HommxLibraryError(
            f"{LIB_PATH} not found: build it with `make -C hommx_amd/csrc` (or __graft_entry__.build()). "
            "hommx_amd has no CPU fallback for the micro-cell solves."
        )
    _share_hip_runtime_with_torch()
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise HommxLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def last_error() -> str:
    return load().hommx_last_error().decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc != 0:
        raise HommxLibraryError(f"{what} failed (code {rc}): {last_error()}")
