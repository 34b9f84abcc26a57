"""The argument checks of hommx_secant_source[_device] on plan-shaped memory: every refusal runs before the plan's device is made
current, so none of them needs a GPU (the manner of tests/test_criterion_abi_host.py)."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib
from hommx_amd.batch import Program
from hommx_amd.expr import OP_ADD, OP_CONST, OP_STORE, OP_X, OP_Y, SecantLaw


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _fake_plan(dim, kind):
    """Plan-shaped memory whose descriptor names `dim` and `kind`: the checks under test read nothing else of it."""
    fake = ctypes.create_string_buffer(4096)
    ctypes.memmove(fake, ctypes.byref(_lib.PlanDesc(dim, 8, kind, 0, 0)), ctypes.sizeof(_lib.PlanDesc))
    return fake


def _program(ops, consts=(), n_comp=2, n_params=0):
    return Program(np.array(ops, dtype=np.uint8).reshape(-1, 2), np.array(consts, dtype=np.float64), n_comp, n_params)


BOTH = [(OP_X, 9), (OP_STORE, 0), (OP_X, 10), (OP_STORE, 1)]  # lam = c[0], mu = c[1] on a plan of t = 3, n_comp = 2


def test_the_symbols_are_exported(lib):
    assert {"hommx_secant_source", "hommx_secant_source_device"} <= set(_lib.EXPORTED_SYMBOLS)
    for name in ("hommx_secant_source", "hommx_secant_source_device"):
        assert getattr(lib, name) is not None
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hommx_hip.h")).read()
    assert "int hommx_secant_source(" in header and "int hommx_secant_source_device(" in header and "} hommx_secant_args;" in header
    assert "#define HOMMX_SECANT_NSTATE 3" in header and _lib.SECANT_NSTATE == 3


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_secant_source_device if device_entry else lib.hommx_secant_source
    tail = (None,) if device_entry else ()
    keep = []

    def call(plan, src, args, n_cells=1):
        rc = fn(plan, n_cells, src, None, None if args is None else ctypes.byref(args), *tail)
        return rc, lib.hommx_last_error().decode()

    def args(prog=None, **kw):
        prog = prog or _program(BOTH)
        keep.append((prog, prog.struct()))
        base = dict(program=ctypes.pointer(keep[-1][1]), n_fields=0, rows=p, points=p, xi=p, max_iter=5, tol=1e-10, relax=1.0, state=p, A_eff=p)
        return _lib.SecantArgs(**dict(base, **kw))

    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    fake = _fake_plan(2, _lib.KIND_ELASTICITY_ISO)  # t = 3, n_comp = 2: a row of 3 + n_fields + 8 entries
    plan = ctypes.addressof(fake)

    def refused(a, text, src=sampled):
        rc, msg = call(plan, src, a)
        assert rc == -1 and text in msg, (text, msg)

    rc, msg = call(None, sampled, args())
    assert rc == -1 and "null plan" in msg
    assert call(plan, None, None, n_cells=0)[0] == 0  # an empty batch reads nothing
    assert call(plan, sampled, args(), n_cells=-1)[0] == -1
    refused(args(), "null source", None)
    refused(args(), "unknown coefficient form 7", ctypes.byref(_lib.CoefSource(form=7, coef=p)))
    rc, msg = call(plan, sampled, None)
    assert rc == -1 and msg == "null arguments"
    refused(args(program=None), "null program")
    for name in ("rows", "xi", "state", "A_eff"):
        refused(args(**{name: None}), "null rows / xi / state / A_eff")
    for kw in ({"strain": p}, {"flux": p}):
        refused(args(**kw), "strain and flux: both or neither")
    # the program: every check of a program, against the plan's n_comp and the wider row
    for nf in (-1, 5):
        refused(args(n_fields=nf), f"n_fields must be 0 .. 4, got {nf}")
    refused(args(_program([(OP_X, 0), (OP_STORE, 0)], n_comp=1)), "n_comp is 1, the plan's coefficient has 2 components")
    refused(args(_program(BOTH + [(OP_X, 0), (OP_STORE, 2)], n_comp=3)), "n_comp is 3, the plan's coefficient has 2 components")
    refused(args(_program([(OP_X, 0), (28, 0), (OP_STORE, 0)] + BOTH[2:])), "unknown opcode 28 at instruction 1")
    refused(args(_program([(OP_X, 11), (OP_STORE, 0)] + BOTH[2:])), "x index 11 out of range [0,11) (the midpoint, 0 fields and the 2 t + n_comp = 8 state entries)")
    refused(args(_program([(OP_X, 13), (OP_STORE, 0)] + BOTH[2:]), n_fields=2), "x index 13 out of range [0,13) (the midpoint, 2 fields")
    refused(args(_program([(OP_CONST, 0), (OP_STORE, 0)] + BOTH[2:])), "constant index 0 out of range [0,0)")
    refused(args(_program([(OP_Y, 2), (OP_STORE, 0)] + BOTH[2:])), "y index 2 out of range [0,2)")
    refused(args(_program([(OP_ADD, 0), (OP_STORE, 0)] + BOTH[2:])), "stack underflow at instruction 0")
    refused(args(_program([(OP_X, 0)] * 17 + [(OP_ADD, 0)] * 16 + [(OP_STORE, 0)] + BOTH[2:])), "stack depth above 16")
    refused(args(_program([(OP_X, 0), (OP_STORE, 2)] + BOTH[2:])), "component index 2 out of range [0,2)")
    refused(args(_program(BOTH + [(OP_X, 1)])), "1 values left on the stack")
    refused(args(_program(BOTH[:2] + BOTH[:2])), "component 0 stored twice")
    refused(args(_program(BOTH[:2])), "component 1 never stored")
    refused(args(_program(BOTH, consts=[1.0], n_params=2)), "n_params is 2, above n_consts (1)")
    refused(args(_program([(OP_Y, 1), (OP_STORE, 0)] + BOTH[2:]), points=None), "null points: the program reads y (instruction 0)")
    # the limits of the iteration
    for bad in (0, -3):
        refused(args(max_iter=bad), f"max_iter must be at least 1, got {bad}")
    refused(args(tol=-1e-3), "tol must be a number >= 0")
    refused(args(tol=float("nan")), "tol must be a number >= 0")
    for bad in (0.0, -0.5, 1.5, float("nan")):
        refused(args(relax=bad), "relax must lie in (0, 1]")
    if device_entry:
        rc, msg = call(plan, sampled, args(), n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg


def test_the_voigt_kind_takes_a_law_of_21_components(lib):
    """A law is no expression coefficient: the 21-component kind is not refused; what comes back for a program of 21 stores is the
    index error of its own row, whose last entry is c[20] = X 35."""
    buf = np.zeros(8)
    p = buf.ctypes.data
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    fake = _fake_plan(3, _lib.KIND_ELASTICITY_VOIGT)  # t = 6, n_comp = 21: a row of 3 + 12 + 21 = 36 entries
    ops, consts = SecantLaw([f"c[{k}]" for k in range(21)]).program(6, 21)
    assert [int(k) for op, k in ops if op == OP_X] == list(range(15, 36)) and [int(k) for op, k in ops if op == OP_STORE] == list(range(21))
    bad = ops.copy()
    bad[40, 1] = 36  # the X of the last component
    prog = Program(bad, consts, 21)
    st = prog.struct()
    a = _lib.SecantArgs(program=ctypes.pointer(st), rows=p, points=p, xi=p, max_iter=1, tol=0.0, relax=1.0, state=p, A_eff=p)
    assert lib.hommx_secant_source(ctypes.addressof(fake), 1, sampled, None, ctypes.byref(a)) == -1
    assert "x index 36 out of range [0,36)" in lib.hommx_last_error().decode()


def test_struct_layout_matches_the_header():
    """hommx_secant_args as the C compiler lays it out: pointers and doubles on 8-byte boundaries."""
    f = {name: getattr(_lib.SecantArgs, name).offset for name, _ in _lib.SecantArgs._fields_}
    assert (f["program"], f["n_fields"], f["rows"], f["points"], f["xi"], f["max_iter"], f["tol"], f["relax"], f["coef_start"]) == \
        (0, 8, 16, 24, 32, 40, 48, 56, 64)
    assert (f["state"], f["A_eff"], f["mean_flux"], f["coef_out"], f["strain"], f["flux"], f["law_values"], f["info"]) == \
        (72, 80, 88, 96, 104, 112, 120, 128)
    assert ctypes.sizeof(_lib.SecantArgs) == 136
