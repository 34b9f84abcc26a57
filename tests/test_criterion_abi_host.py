"""The argument checks of hommx_criterion_source[_device] on plan-shaped memory: every refusal runs before the plan's device is made
current, so none of them needs a GPU (the manner of tests/test_reconstruct_source_host.py)."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib
from hommx_amd.batch import Program
from hommx_amd.expr import OP_ADD, OP_CONST, OP_STORE, OP_X, OP_Y, Criterion


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


def _program(ops, consts=(), n_comp=1, n_params=0):
    return Program(np.array(ops, dtype=np.uint8).reshape(-1, 2), np.array(consts, dtype=np.float64), n_comp, n_params)


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_criterion_source_device if device_entry else lib.hommx_criterion_source
    tail = (None,) if device_entry else ()
    keep = []

    def call(plan, src, args, n_cells=1):
        rc = fn(plan, n_cells, src, None, None if args is None else ctypes.byref(args), *tail)
        return rc, lib.hommx_last_error().decode()

    def args(prog=None, **kw):
        prog = prog or _program([(OP_X, 3 + 0 + 2 + 0), (OP_STORE, 0)])  # s[0] on a plan of t = 2 .. 3
        keep.append((prog, prog.struct()))
        base = dict(program=ctypes.pointer(keep[-1][1]), n_fields=0, rows=p, points=p, xi=p, threshold=1.0, crit=p)
        return _lib.CriterionArgs(**dict(base, **kw))

    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    fake = _fake_plan(2, _lib.KIND_ELASTICITY_ISO)  # t = 3, n_comp = 2: a row of 3 + n_fields + 8 entries
    plan = ctypes.addressof(fake)
    assert lib.hommx_plan_kind(plan) == _lib.KIND_ELASTICITY_ISO

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
    for name in ("rows", "xi", "crit"):
        refused(args(**{name: None}), "null rows / xi / crit")
    for kw in ({"strain": p}, {"flux": p}):
        refused(args(**kw), "strain and flux: both or neither")
    # the program: every check of a program source, against one component and the wider row
    for nf in (-1, 5):
        refused(args(n_fields=nf), f"n_fields must be 0 .. 4, got {nf}")
    refused(args(_program([(OP_X, 0), (OP_STORE, 0)], n_comp=2)), "n_comp is 2, a criterion has one component")
    refused(args(_program([(OP_X, 0), (28, 0), (OP_STORE, 0)])), "unknown opcode 28 at instruction 1")
    refused(args(_program([(OP_X, 11), (OP_STORE, 0)])), "x index 11 out of range [0,11) (the midpoint, 0 fields and the 2 t + n_comp = 8 state entries)")
    refused(args(_program([(OP_X, 13), (OP_STORE, 0)]), n_fields=2), "x index 13 out of range [0,13) (the midpoint, 2 fields")
    refused(args(_program([(OP_CONST, 0), (OP_STORE, 0)])), "constant index 0 out of range [0,0)")
    refused(args(_program([(OP_Y, 2), (OP_STORE, 0)])), "y index 2 out of range [0,2)")
    refused(args(_program([(OP_ADD, 0), (OP_STORE, 0)])), "stack underflow at instruction 0")
    refused(args(_program([(OP_X, 0)] * 17 + [(OP_ADD, 0)] * 16 + [(OP_STORE, 0)])), "stack depth above 16")
    refused(args(_program([(OP_X, 0), (OP_STORE, 1)])), "component index 1 out of range [0,1)")
    refused(args(_program([(OP_X, 0), (OP_X, 1), (OP_STORE, 0)])), "1 values left on the stack")
    refused(args(_program([(OP_X, 0), (OP_STORE, 0), (OP_X, 1), (OP_STORE, 0)])), "component 0 stored twice")
    refused(args(_program([(OP_X, 0), (OP_STORE, 0)], consts=[1.0], n_params=2)), "n_params is 2, above n_consts (1)")
    refused(args(_program([(OP_Y, 1), (OP_STORE, 0)]), points=None), "null points: the program reads y (instruction 0)")
    refused(args(threshold=float("nan")), "the threshold is NaN")
    # a load: the refusals of hommx_loads_source for its code and source, and the shared code
    refused(args(has_load=1, per_cell=3, P=p), "unknown load code 3 in per_cell")
    refused(args(has_load=1, per_cell=8, P=p), "unknown load code 8 in per_cell")
    refused(args(has_load=1, per_cell=_lib.LOADS_SHARED, P=p), "a criterion takes its load per cell")
    refused(args(has_load=1, per_cell=_lib.LOADS_PER_CELL), "null P")
    refused(args(has_load=1, per_cell=_lib.LOADS_PROGRAM), "HOMMX_LOADS_PROGRAM needs P_source")
    other = _lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p)
    refused(args(has_load=1, per_cell=_lib.LOADS_PROGRAM, P_source=ctypes.pointer(other)), "P_source must be a HOMMX_COEF_PROGRAM source, got form 0")
    scalar = _program([(OP_X, 0), (OP_STORE, 0)])
    keep.append(scalar.struct())
    load = _lib.CoefSource(form=_lib.COEF_PROGRAM, n_q=1, table=p, weights=p, params=p, program=ctypes.pointer(keep[-1]))
    refused(args(has_load=1, per_cell=_lib.LOADS_PROGRAM | _lib.LOADS_EIGENSTRAIN, P_source=ctypes.pointer(load)),
            "P_source: program: n_comp is 1, a load of this plan has t = 3 components")
    if device_entry:
        rc, msg = call(plan, sampled, args(), n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg


def test_the_voigt_kind_takes_a_criterion_and_every_ready_made_text_passes_its_plan(lib):
    """A criterion is no coefficient: the 21-component kind is not refused (what comes back is the index error of its own row, whose
    last entry is c[20] = X 35)."""
    buf = np.zeros(8)
    p = buf.ctypes.data
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    fake = _fake_plan(3, _lib.KIND_ELASTICITY_VOIGT)  # t = 6, n_comp = 21: a row of 3 + 12 + 21 = 36 entries
    ops, consts = Criterion("c[20] + s[5]").program(6, 21)
    assert [k for op, k in ops if op == OP_X] == [35, 14]
    prog = _program([(OP_X, 36), (OP_STORE, 0)])
    st = prog.struct()
    a = _lib.CriterionArgs(program=ctypes.pointer(st), rows=p, points=p, xi=p, threshold=1.0, crit=p)
    assert lib.hommx_criterion_source(ctypes.addressof(fake), 1, sampled, None, ctypes.byref(a)) == -1
    assert "x index 36 out of range [0,36)" in lib.hommx_last_error().decode()


def test_struct_layout_matches_the_header():
    """hommx_criterion_args as the C compiler lays it out: pointers and the double on 8-byte boundaries."""
    f = {name: getattr(_lib.CriterionArgs, name).offset for name, _ in _lib.CriterionArgs._fields_}
    assert (f["program"], f["n_fields"], f["rows"], f["points"], f["xi"], f["threshold"], f["has_load"], f["per_cell"], f["P"]) == \
        (0, 8, 16, 24, 32, 40, 48, 52, 56)
    assert (f["P_source"], f["crit"], f["values"], f["strain"], f["flux"], f["A_eff"], f["info"]) == (64, 72, 80, 88, 96, 104, 112)
    assert ctypes.sizeof(_lib.CriterionArgs) == 120
