"""The program form of a coefficient source at the C ABI, on the CPU: the library validates the whole program on the host, before the
plan's device is made current, reading nothing of the plan but its descriptor -- so plan-shaped memory that holds only a hommx_plan_desc
reaches every check (the manner of test_solve_abi_host.py).  Every call here is a faulty one or an empty batch: none may get past the
checks.  No GPU needed."""

import ctypes as C
import os

import numpy as np
import pytest

from hommx_amd import _lib, expr
from hommx_amd.batch import Program
from test_reconstruct_source_host import _fake_plan


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


BUF = np.zeros(64)
P = BUF.ctypes.data

# entry -> the arguments after the source (every pointer set)
ENTRIES = {
    "hommx_solve_batch_source": (None, P, None),
    "hommx_solve_batch_source_device": (None, P, None, None),
    "hommx_expand_source": (P,),
    "hommx_expand_source_device": (P, None),
    "hommx_sensitivity_source": (None, "sens"),
    "hommx_sensitivity_source_device": (None, "sens", None),
}
SENS = _lib.SensArgs(1, 0, P, P, None, None, None, None)


def call(lib, entry, plan, n_cells, src, args=None):
    args = ENTRIES[entry] if args is None else args
    rc = getattr(lib, entry)(plan, n_cells, src, *[C.byref(SENS) if a == "sens" else a for a in args])
    return rc, lib.hommx_last_error().decode()


def source(ops, consts=(), n_comp=1, n_q=3, keep=[], **over):
    """A program source with every pointer set; ``over`` replaces members of the source (``program=None``: no program) or, with a
    ``prog_`` prefix, of the program struct."""
    prog = Program(np.array(ops, dtype=np.uint8).reshape(-1, 2), np.array(consts, dtype=np.float64), n_comp)
    g = prog.struct()
    for k in [k for k in over if k.startswith("prog_")]:
        setattr(g, k[5:], over.pop(k))
    src = _lib.CoefSource(form=_lib.COEF_PROGRAM, n_q=n_q, table=P, weights=P, params=P, program=C.pointer(g))
    for k, v in over.items():
        setattr(src, k, v)
    keep.append((prog, g, src))
    return C.byref(src)


Y0, Y1, ADD, ST0, ST1 = (expr.OP_Y, 0), (expr.OP_Y, 1), (expr.OP_ADD, 0), (expr.OP_STORE, 0), (expr.OP_STORE, 1)
GOOD = [Y0, Y1, ADD, ST0]
DEEP = [Y0] * (expr.MAX_STACK + 1) + [ADD] * expr.MAX_STACK + [ST0]

# (what the test is called, keyword arguments of source(), the plan's kind, the text the library names the fault with)
FAULTS = [
    ("unknown opcode", dict(ops=[Y0, (28, 0), ST0]), 0, "unknown opcode 28 at instruction 1"),
    ("unknown opcode 255", dict(ops=[(255, 0), ST0]), 0, "unknown opcode 255"),
    ("constant index", dict(ops=[(expr.OP_CONST, 2), ST0], consts=[1.0, 2.0]), 0, "constant index 2 out of range [0,2)"),
    ("constant without table", dict(ops=[(expr.OP_CONST, 0), ST0]), 0, "constant index 0 out of range [0,0)"),
    ("x index", dict(ops=[(expr.OP_X, 3), ST0]), 0, "x index 3 out of range [0,3)"),
    ("y index", dict(ops=[(expr.OP_Y, 2), ST0]), 0, "y index 2 out of range [0,2)"),  # the fake plan is 2D
    ("underflow binary", dict(ops=[Y0, ADD, ST0]), 0, "stack underflow at instruction 1"),
    ("underflow store", dict(ops=[ST0]), 0, "stack underflow at instruction 0"),
    ("underflow select", dict(ops=[Y0, Y0, (expr.OP_SELECT, 0), ST0]), 0, "stack underflow at instruction 2"),
    ("underflow dup", dict(ops=[(expr.OP_DUP, 0), ST0]), 0, "stack underflow at instruction 0"),
    ("too deep", dict(ops=DEEP), 0, "stack depth above 16 at instruction 16"),
    ("left on the stack", dict(ops=[Y0, Y1, ST0]), 0, "1 values left on the stack at the end"),
    ("stored twice", dict(ops=[Y0, ST0, Y1, ST0], n_comp=2), _lib.KIND_ELASTICITY_ISO, "component 0 stored twice (instruction 3)"),
    ("never stored", dict(ops=[Y0, ST1], n_comp=2), _lib.KIND_ELASTICITY_ISO, "component 0 never stored"),
    ("component index", dict(ops=[Y0, ST1]), 0, "component index 1 out of range [0,1)"),
    ("n_comp of the plan", dict(ops=[Y0, ST0, Y1, ST1], n_comp=2), 0, "n_comp is 2, the plan's coefficient has 1 components"),
    ("n_comp of the matrix plan", dict(ops=GOOD), _lib.KIND_POISSON_MATRIX, "n_comp is 1, the plan's coefficient has 3 components"),
    ("n_ops above 128", dict(ops=GOOD, prog_n_ops=129), 0, "n_ops must be 1 .. 128, got 129"),
    ("n_ops zero", dict(ops=GOOD, prog_n_ops=0), 0, "n_ops must be 1 .. 128, got 0"),
    ("n_consts above 32", dict(ops=GOOD, prog_n_consts=33), 0, "n_consts must be 0 .. 32, got 33"),
    ("voigt kind", dict(ops=GOOD), _lib.KIND_ELASTICITY_VOIGT, "not supported for the 21-component Voigt kind"),
    ("null program", dict(ops=GOOD, program=None), 0, "null program"),
    ("null ops", dict(ops=GOOD, prog_ops=None), 0, "null program ops / consts"),
    ("null consts", dict(ops=[(expr.OP_CONST, 0), ST0], consts=[1.0], prog_consts=None), 0, "null program ops / consts"),
    ("n_q", dict(ops=GOOD, n_q=0), 0, "program source needs n_q >= 1"),
    ("null table", dict(ops=GOOD, table=None), 0, "null table / weights / params"),
    ("null weights", dict(ops=GOOD, weights=None), 0, "null table / weights / params"),
    ("null params", dict(ops=GOOD, params=None), 0, "null table / weights / params"),
]


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("name,kw,kind,text", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_fault_is_named(lib, entry, name, kw, kind, text):
    fake = _fake_plan(kind)
    rc, msg = call(lib, entry, C.addressof(fake), 1, source(**kw))
    assert rc == -1 and text in msg, (rc, msg)


def test_a_program_at_the_limits_passes_the_validation(lib):
    """Depth 16 and 128 instructions are accepted: the call gets as far as the entry's own pointer check."""
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    at_depth = [Y0] * expr.MAX_STACK + [ADD] * (expr.MAX_STACK - 1) + [ST0]
    longest = [Y0] + [(expr.OP_NEG, 0)] * (expr.MAX_OPS - 2) + [ST0]
    for ops in (at_depth, longest, expr.Expression("1.1 + x[0] + sin(2*pi*y[0])").program()[0]):
        consts = [1.1, 2 * np.pi]
        rc, msg = call(lib, "hommx_expand_source", C.addressof(fake), 1, source(ops=ops, consts=consts), (None,))
        assert rc == -1 and msg == "null coef_out", (rc, msg)
        rc, msg = call(lib, "hommx_solve_batch_source_device", C.addressof(fake), 1, source(ops=ops, consts=consts), (None, None, None, None))
        assert rc == -1 and msg == "null A_eff", (rc, msg)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_plan_batch_size_and_source(lib, entry):
    good = source(ops=GOOD)
    for n_cells in (1, 0, -1):  # a null plan is an error even for an empty batch
        rc, msg = call(lib, entry, None, n_cells, good)
        assert rc == -1 and "null plan" in msg, (n_cells, rc, msg)
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan = C.addressof(fake)
    rc, msg = call(lib, entry, plan, -1, good)
    assert rc == -1 and "negative n_cells" in msg
    rc, msg = call(lib, entry, plan, 1, None)
    assert rc == -1 and "null source" in msg
    rc, msg = call(lib, entry, plan, 1, C.byref(_lib.CoefSource(form=4, coef=P)))
    assert rc == -1 and "unknown coefficient form 4" in msg
    # an empty batch reads no pointer: neither the source, nor the program of a source, nor the arguments
    nothing = tuple(None for _ in ENTRIES[entry])
    assert call(lib, entry, plan, 0, None, nothing)[0] == 0
    assert call(lib, entry, plan, 0, source(ops=GOOD, program=None, table=None, weights=None, params=None), nothing)[0] == 0
    assert call(lib, entry, plan, 0, source(ops=[(77, 9)]), nothing)[0] == 0


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.endswith("_device")])
def test_batch_too_large_for_one_launch(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    rc, msg = call(lib, entry, C.addressof(fake), 2**31, source(ops=GOOD))
    assert rc == -1 and "too large for one launch" in msg, (rc, msg)


def test_the_other_forms_go_through_the_new_entries_checks(lib):
    """The generic entries take every form with the checks (and texts) the form has everywhere else."""
    fake = _fake_plan(_lib.KIND_POISSON_MATRIX)
    for entry in ("hommx_solve_batch_source", "hommx_expand_source_device"):
        rc, msg = call(lib, entry, C.addressof(fake), 1, C.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED)))
        assert rc == -1 and msg == "null coef"
        rc, msg = call(lib, entry, C.addressof(fake), 1, C.byref(_lib.CoefSource(form=_lib.COEF_TWO_PHASE, mask=P)))
        assert rc == -1 and msg == "null mask / values"
        rc, msg = call(lib, entry, C.addressof(fake), 1, C.byref(_lib.CoefSource(form=_lib.COEF_SEPARABLE, table=P, params=P)))
        assert rc == -1 and "separable samplers are defined for" in msg


def test_struct_layout():
    """`program` is appended: every member a caller of the shorter struct knows keeps its offset."""
    S = _lib.CoefSource
    assert [getattr(S, f).offset for f in ("form", "family", "n_q", "reserved", "coef", "mask", "values", "table", "weights", "params",
                                           "program")] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert C.sizeof(S) == 72 and C.sizeof(_lib.CoefProgram) == 32
    assert (_lib.COEF_PROGRAM, _lib.PROGRAM_MAX_OPS, _lib.PROGRAM_MAX_CONSTS, _lib.PROGRAM_MAX_STACK) == (3, expr.MAX_OPS, expr.MAX_CONSTS, expr.MAX_STACK)
