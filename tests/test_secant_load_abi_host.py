"""The argument checks of the four entries that take a load beside a law (hommx_secant_load_source[_device],
hommx_secant_tangent_load_source[_device]) on plan-shaped memory: every refusal runs before the plan's device is made
current, so none of them needs a GPU (the manner of tests/test_secant_abi_host.py)."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib
from hommx_amd.expr import OP_STORE, OP_X
from test_secant_abi_host import BOTH, _fake_plan, _program

NAMES = ("hommx_secant_load_source", "hommx_secant_load_source_device", "hommx_secant_tangent_load_source",
         "hommx_secant_tangent_load_source_device")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_the_symbols_are_exported(lib):
    assert set(NAMES) <= set(_lib.EXPORTED_SYMBOLS)
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hommx_hip.h")).read()
    for name in NAMES:
        assert getattr(lib, name) is not None and f"int {name}(" in header
    assert "} hommx_secant_load_args;" in header


def test_struct_layout_matches_the_header():
    """hommx_secant_load_args as the C compiler lays it out: an int32 padded to 8 and two pointers; the structs beside it are untouched."""
    f = {name: getattr(_lib.SecantLoadArgs, name).offset for name, _ in _lib.SecantLoadArgs._fields_}
    assert [f[n] for n in ("per_cell", "P", "P_source")] == [0, 8, 16]
    assert ctypes.sizeof(_lib.SecantLoadArgs) == 24
    assert ctypes.sizeof(_lib.SecantArgs) == 136 and ctypes.sizeof(_lib.SecantTangentArgs) == 48 and ctypes.sizeof(_lib.HistoryArgs) == 24


@pytest.mark.parametrize("device_entry", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("tangent", [False, True], ids=["secant", "tangent"])
def test_abi_argument_checks(lib, tangent, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = getattr(lib, NAMES[2 * tangent + device_entry])
    tail = (None,) if device_entry else ()
    keep = []
    fake = _fake_plan(2, _lib.KIND_ELASTICITY_ISO)  # t = 3, n_comp = 2: a row of 3 + n_fields + 8 entries; its tangent kind is Voigt
    plan = ctypes.addressof(fake)
    sibling = _fake_plan(2, _lib.KIND_ELASTICITY_VOIGT)
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    per_cell = _lib.SecantLoadArgs(_lib.LOADS_PER_CELL, p, None)

    def secant(prog=None, **kw):
        prog = prog or _program(BOTH)
        keep.append((prog, prog.struct()))
        base = dict(program=ctypes.pointer(keep[-1][1]), n_fields=0, rows=p, points=p, xi=p, max_iter=5, tol=1e-10, relax=1.0, state=p, A_eff=p)
        keep.append(_lib.SecantArgs(**dict(base, **kw)))
        return keep[-1]

    def args(s=None, **kw):
        s = s if s is not None else secant()
        if not tangent:
            return s
        keep.append(_lib.SecantTangentArgs(**dict(dict(secant=ctypes.pointer(s), tangent_plan=ctypes.addressof(sibling), tangent=p, asymmetry=p), **kw)))
        return keep[-1]

    def call(pl, src, a, hist, load, n_cells=1):
        ref = lambda x: None if x is None else ctypes.byref(x)
        rc = fn(pl, n_cells, src, None, ref(a), ref(hist), ref(load), *tail)
        return rc, lib.hommx_last_error().decode()

    def refused(text, a=None, hist=None, load=per_cell, src=sampled):
        rc, msg = call(plan, src, a if a is not None else args(), hist, load)
        assert rc == -1 and text in msg, (text, msg)

    # what opens every entry of the family
    rc, msg = call(None, sampled, args(), None, per_cell)
    assert rc == -1 and "null plan" in msg
    assert call(plan, None, None, None, None, n_cells=0)[0] == 0  # an empty batch reads nothing
    assert call(plan, sampled, args(), None, per_cell, n_cells=-1)[0] == -1
    refused("null source", src=None)
    refused("unknown coefficient form 7", src=ctypes.byref(_lib.CoefSource(form=7, coef=p)))
    rc, msg = call(plan, sampled, None, None, per_cell)
    assert rc == -1 and msg == "null arguments"
    # everything the entry without a load refuses, through the same checks
    refused("null program", args(secant(program=None)))
    for name in ("rows", "xi", "state", "A_eff"):
        refused("null rows / xi / state / A_eff", args(secant(**{name: None})))
    refused("strain and flux: both or neither", args(secant(strain=p)))
    refused("n_fields must be 0 .. 4, got 5", args(secant(n_fields=5)))
    refused("n_comp is 1, the plan's coefficient has 2 components", args(secant(_program([(OP_X, 0), (OP_STORE, 0)], n_comp=1))))
    refused("component 1 never stored", args(secant(_program(BOTH[:2]))))
    refused("max_iter must be at least 1, got 0", args(secant(max_iter=0)))
    refused("tol must be a number >= 0", args(secant(tol=float("nan"))))
    refused("relax must lie in (0, 1]", args(secant(relax=1.5)))
    if tangent:
        refused("null tangent_plan / tangent / asymmetry", args(tangent=None))
        refused("tangent_plan is the plan itself", args(tangent_plan=plan))
        refused("the law reads s[0] (instruction 0)", args(secant(_program([(OP_X, 6), (OP_STORE, 0)] + BOTH[2:]))))
    # the optional history: NULL is none, a struct is checked as the history entries check it
    refused("n_history must be 1 .. 4, got 0", hist=_lib.HistoryArgs(0, p, p + 8))
    refused("null history_in / history_out", hist=_lib.HistoryArgs(1, None, p))
    refused("history_in and history_out are the same array", hist=_lib.HistoryArgs(1, p, p))
    # the load
    refused("null load arguments", load=None)
    for code in (3, 7, 8, 16, -1):
        refused(f"unknown load code {code} in per_cell", load=_lib.SecantLoadArgs(code, p, None))
    for flag in (0, _lib.LOADS_EIGENSTRAIN):
        refused("a law takes its load per cell (HOMMX_LOADS_PER_CELL) or as a program (HOMMX_LOADS_PROGRAM)",
                load=_lib.SecantLoadArgs(_lib.LOADS_SHARED | flag, p, None))
        refused("null P", load=_lib.SecantLoadArgs(_lib.LOADS_PER_CELL | flag, None, None))
        refused("HOMMX_LOADS_PROGRAM needs P_source", load=_lib.SecantLoadArgs(_lib.LOADS_PROGRAM | flag, p, None))
        other = _lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p)
        refused("P_source must be a HOMMX_COEF_PROGRAM source, got form 0", load=_lib.SecantLoadArgs(_lib.LOADS_PROGRAM | flag, None, ctypes.pointer(other)))
    # a load that passes every check up to the device, which plan-shaped memory cannot serve -- so ask for too much
    if device_entry:
        rc, msg = call(plan, sampled, args(secant(_program([(OP_X, 5), (OP_STORE, 0)] + BOTH[2:]))), None, per_cell, n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg
