"""The load codes of hommx_load_args at the C ABI, on the CPU: HOMMX_LOADS_PROGRAM (the load comes from a program source of its own,
P_source) and the flag HOMMX_LOADS_EIGENSTRAIN.  Every check runs on the host before the plan's device is made current and reads nothing
of the plan but its descriptor, so plan-shaped memory that holds only a hommx_plan_desc reaches all of them (the manner of
test_program_abi_host.py).  A call that passes them goes on to make the plan's device current: where there is none it fails there, with
a text that is none of the checks' -- the one test that sends such calls names a device no machine has.  No GPU needed."""

import ctypes as C
import os

import numpy as np
import pytest

from hommx_amd import _lib, expr
from hommx_amd.batch import Program
from test_reconstruct_source_host import _fake_plan

BUF = np.zeros(64)
P = BUF.ctypes.data
T = {_lib.KIND_POISSON_SCALAR: 2, _lib.KIND_POISSON_MATRIX: 2, _lib.KIND_ELASTICITY_ISO: 3, _lib.KIND_ELASTICITY_VOIGT: 3}  # the fake plan is 2D
Y0, Y1, ADD = (expr.OP_Y, 0), (expr.OP_Y, 1), (expr.OP_ADD, 0)
ST = [(expr.OP_STORE, c) for c in range(6)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def good_ops(t):
    return [op for c in range(t) for op in (Y0, Y1, ADD, ST[c])]


def load_source(ops, consts=(), n_comp=2, n_q=3, keep=[], **over):
    """A program source for P_source with every pointer set; ``over`` replaces members of the source or, with a ``prog_`` prefix, of the
    program struct."""
    prog = Program(np.array(ops, dtype=np.uint8).reshape(-1, 2), np.array(consts, dtype=np.float64), n_comp)
    g = prog.struct()
    for k in [k for k in over if k.startswith("prog_")]:
        setattr(g, k[5:], over.pop(k))
    src = _lib.CoefSource(form=_lib.COEF_PROGRAM, n_q=n_q, table=P, weights=P, params=P, program=C.pointer(g))
    for k, v in over.items():
        setattr(src, k, v)
    keep.append((prog, g, src))
    return C.pointer(src)


def call(lib, device_entry, plan, args, n_cells=1):
    fn = lib.hommx_loads_source_device if device_entry else lib.hommx_loads_source
    sampled = C.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=P))
    rc = fn(plan, n_cells, sampled, None, C.byref(args), *((None,) if device_entry else ()))
    return rc, lib.hommx_last_error().decode()


def load_args(**kw):
    return _lib.LoadArgs(**dict(dict(n_loads=1, per_cell=_lib.LOADS_PROGRAM, P=None, P_eff=P), **kw))


def test_constants_and_layout():
    assert (_lib.LOADS_SHARED, _lib.LOADS_PER_CELL, _lib.LOADS_PROGRAM, _lib.LOADS_EIGENSTRAIN) == (0, 1, 2, 4)
    A = _lib.LoadArgs
    # P_source is appended: every member a caller of the shorter struct knows keeps its offset
    assert [getattr(A, f).offset for f in ("n_loads", "per_cell", "P", "P_eff", "A_eff", "energy", "stats", "strain", "flux", "correctors",
                                           "info", "P_source")] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80]
    assert C.sizeof(A) == 88
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hommx_hip.h")).read()
    for name, value in (("SHARED", 0), ("PER_CELL", 1), ("PROGRAM", 2), ("EIGENSTRAIN", 4)):
        assert f"#define HOMMX_LOADS_{name} {value}" in " ".join(header.split())


@pytest.mark.parametrize("device_entry", [False, True])
@pytest.mark.parametrize("kind", list(T))
def test_unknown_codes(lib, device_entry, kind):
    plan = _fake_plan(kind)
    for code in (3, 7, 8, 9, 16, -1, 2 | 8):
        rc, msg = call(lib, device_entry, C.addressof(plan), load_args(per_cell=code, P=P, P_source=load_source(good_ops(T[kind]), n_comp=T[kind])))
        assert rc == -1 and f"unknown load code {code} in per_cell" in msg and "HOMMX_LOADS_EIGENSTRAIN" in msg, (code, rc, msg)


# (name, keyword arguments of load_source() -- t: the plan's tensor size --, members of the argument struct, the text)
def _faults(t):
    ok = dict(ops=good_ops(t), n_comp=t)
    return [
        ("null P_source", None, {}, "HOMMX_LOADS_PROGRAM needs P_source"),
        ("another form", dict(ok, form=_lib.COEF_SAMPLED), {}, f"P_source must be a HOMMX_COEF_PROGRAM source, got form {_lib.COEF_SAMPLED}"),
        ("two-phase form", dict(ok, form=_lib.COEF_TWO_PHASE), {}, f"P_source must be a HOMMX_COEF_PROGRAM source, got form {_lib.COEF_TWO_PHASE}"),
        ("n_loads", ok, dict(n_loads=2), "HOMMX_LOADS_PROGRAM takes n_loads == 1 (callers loop for more), got 2"),
        ("n_comp of the coefficient", dict(ops=good_ops(1), n_comp=1), {}, f"P_source: program: n_comp is 1, a load of this plan has t = {t} components"),
        ("n_comp above t", dict(ops=good_ops(t + 1), n_comp=t + 1), {}, f"n_comp is {t + 1}, a load of this plan has t = {t} components"),
        ("null program", dict(ok, program=None), {}, "P_source: null program"),
        ("null ops", dict(ok, prog_ops=None), {}, "null program ops / consts"),
        ("null consts", dict(ops=[(expr.OP_CONST, 0), ST[0]] + good_ops(t)[4:], n_comp=t, consts=[1.0], prog_consts=None), {}, "null program ops / consts"),
        ("n_ops", dict(ok, prog_n_ops=129), {}, "n_ops must be 1 .. 128, got 129"),
        ("n_consts", dict(ok, prog_n_consts=33), {}, "n_consts must be 0 .. 32, got 33"),
        ("n_params", dict(ok, prog_n_params=5), {}, "n_params must be 0 .. 4, got 5"),
        ("n_params above n_consts", dict(ok, prog_n_params=1), {}, "n_params is 1, above n_consts (0)"),
        ("n_fields", dict(ok, n_fields=5), {}, "n_fields must be 0 .. 4, got 5"),
        ("n_q", dict(ok, n_q=0), {}, "program source needs n_q >= 1"),
        ("null table", dict(ok, table=None), {}, "null table / weights / params"),
        ("null weights", dict(ok, weights=None), {}, "null table / weights / params"),
        ("null rows", dict(ok, params=None), {}, "null table / weights / params"),
        ("unknown opcode", dict(ops=[Y0, (28, 0), ST[0]] + good_ops(t)[4:], n_comp=t), {}, "unknown opcode 28 at instruction 1"),
        ("constant index", dict(ops=[(expr.OP_CONST, 1), ST[0]] + good_ops(t)[4:], n_comp=t, consts=[1.0]), {}, "constant index 1 out of range [0,1)"),
        ("x index", dict(ops=[(expr.OP_X, 3), ST[0]] + good_ops(t)[4:], n_comp=t), {}, "x index 3 out of range [0,3)"),
        ("x index with fields", dict(ops=[(expr.OP_X, 5), ST[0]] + good_ops(t)[4:], n_comp=t, n_fields=2), {}, "x index 5 out of range [0,5) (the midpoint and 2 fields)"),
        ("y index", dict(ops=[(expr.OP_Y, 2), ST[0]] + good_ops(t)[4:], n_comp=t), {}, "y index 2 out of range [0,2)"),
        ("underflow", dict(ops=[Y0, ADD, ST[0]] + good_ops(t)[4:], n_comp=t), {}, "stack underflow at instruction 1"),
        ("too deep", dict(ops=[Y0] * 17 + [ADD] * 16 + [ST[0]] + good_ops(t)[4:], n_comp=t), {}, "stack depth above 16 at instruction 16"),
        ("left on the stack", dict(ops=[Y0] + good_ops(t), n_comp=t), {}, "1 values left on the stack at the end"),
        ("stored twice", dict(ops=good_ops(t)[:4] + good_ops(t)[:4], n_comp=t), {}, "component 0 stored twice (instruction 7)"),
        ("never stored", dict(ops=good_ops(t)[4:], n_comp=t), {}, "component 0 never stored"),
        ("component index", dict(ops=good_ops(t)[:3] + [ST[t]] + good_ops(t)[4:], n_comp=t), {}, f"component index {t} out of range [0,{t})"),
        ("null P_eff", ok, dict(P_eff=None), "null P_eff"),
        ("strain without flux", ok, dict(strain=P), "strain and flux: both or neither"),
    ]


NAMES = [f[0] for f in _faults(2)]


@pytest.mark.parametrize("device_entry", [False, True])
@pytest.mark.parametrize("eigenstrain", [0, _lib.LOADS_EIGENSTRAIN])
@pytest.mark.parametrize("kind", list(T))  # the Voigt kind among them: a load program is not a coefficient program
@pytest.mark.parametrize("which", range(len(NAMES)), ids=NAMES)
def test_every_fault_of_a_program_load_is_named(lib, device_entry, eigenstrain, kind, which):
    name, src_kw, arg_kw, text = _faults(T[kind])[which]
    plan = _fake_plan(kind)
    src = None if src_kw is None else load_source(**src_kw)
    rc, msg = call(lib, device_entry, C.addressof(plan), load_args(per_cell=_lib.LOADS_PROGRAM | eigenstrain, P_source=src, **arg_kw))
    assert rc == -1 and text in msg, (name, rc, msg)


@pytest.mark.parametrize("device_entry", [False, True])
def test_array_codes_check_what_they_checked(lib, device_entry):
    plan = _fake_plan(_lib.KIND_ELASTICITY_ISO)
    for code in (_lib.LOADS_SHARED, _lib.LOADS_PER_CELL, _lib.LOADS_SHARED | _lib.LOADS_EIGENSTRAIN, _lib.LOADS_PER_CELL | _lib.LOADS_EIGENSTRAIN):
        for kw in (dict(P=None), dict(P=P, P_eff=None)):
            rc, msg = call(lib, device_entry, C.addressof(plan), load_args(per_cell=code, **dict(dict(P=P), **kw)))
            assert rc == -1 and msg == "null P / P_eff", (code, rc, msg)
        for nl in (0, 4):
            rc, msg = call(lib, device_entry, C.addressof(plan), load_args(per_cell=code, P=P, n_loads=nl))
            assert rc == -1 and msg == f"n_loads must be 1 .. 3 (the tensor size of the plan), got {nl}"
    # an empty batch reads nothing, whatever the code says
    assert call(lib, device_entry, C.addressof(plan), load_args(per_cell=99, P_source=None), n_cells=0)[0] == 0


def _plan_without_device(kind):
    """Plan-shaped memory like ``_fake_plan``'s whose descriptor names a device no machine has: a call that passes every check fails
    where it makes that device current, on a machine with GPUs as on one without."""
    fake = C.create_string_buffer(4096)
    C.memmove(fake, C.byref(_lib.PlanDesc(2, 8, kind, 1 << 20, 0)), C.sizeof(_lib.PlanDesc))
    return fake


CHECK_TEXTS = ("unknown load code", "P_source", "n_loads", "null P", "program", "strain and flux", "null source", "null coef", "null arguments")


@pytest.mark.parametrize("device_entry", [False, True])
def test_what_passes_the_checks_gets_as_far_as_the_device(lib, device_entry):
    """Codes 0 and 1 (alone or as eigenstrains) with a GARBAGE P_source pass the validation -- the member is never read --, and so does a
    good program load: each call fails only where the plan's device is made current, with the runtime's text."""
    garbage = C.cast(C.c_void_p(0x10), C.POINTER(_lib.CoefSource))  # reading it would fault
    for kind, t in T.items():
        plan = _plan_without_device(kind)
        for code in (0, 1, 4, 5):
            rc, msg = call(lib, device_entry, C.addressof(plan), load_args(per_cell=code, P=P, P_source=garbage))
            assert rc != 0 and not any(text in msg for text in CHECK_TEXTS), (kind, code, rc, msg)
        for code in (2, 6):
            rc, msg = call(lib, device_entry, C.addressof(plan), load_args(per_cell=code, P_source=load_source(good_ops(t), n_comp=t)))
            assert rc != 0 and not any(text in msg for text in CHECK_TEXTS), (kind, code, rc, msg)
