"""The argument checks of the four history entries (hommx_secant_history_source[_device], hommx_secant_tangent_history_source[_device];
DESIGN 4.17) on plan-shaped memory: every refusal runs before the plan's device is made current, so none of them needs a GPU (the
manner of tests/test_secant_abi_host.py).  The exported symbols, the layout of hommx_history_args, the two older structs unchanged."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib
from hommx_amd.expr import OP_STORE, OP_X
from test_secant_abi_host import BOTH, _fake_plan, _program

NAMES = ("hommx_secant_history_source", "hommx_secant_history_source_device", "hommx_secant_tangent_history_source",
         "hommx_secant_tangent_history_source_device")
# lam = c[0], mu = c[1], h0' = h[0], h1' = h[1] on a plan of t = 3, n_comp = 2 with two history variables: a row of 3 + 8 + 2 entries
HIST = BOTH + [(OP_X, 11), (OP_STORE, 2), (OP_X, 12), (OP_STORE, 3)]


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
    assert "} hommx_history_args;" in header and "#define HOMMX_SECANT_MAX_HISTORY 4" in header and _lib.SECANT_MAX_HISTORY == 4
    assert "history_in == history_out" in header  # the header says why: the input is read in every round


def test_struct_layouts():
    """hommx_history_args as the C compiler lays it out -- an int32 padded to 8, two pointers --; the two older structs untouched."""
    f = {name: getattr(_lib.HistoryArgs, name).offset for name, _ in _lib.HistoryArgs._fields_}
    assert [f[n] for n in ("n_history", "history_in", "history_out")] == [0, 8, 16] and ctypes.sizeof(_lib.HistoryArgs) == 24
    assert ctypes.sizeof(_lib.SecantArgs) == 136 and ctypes.sizeof(_lib.SecantTangentArgs) == 48


@pytest.mark.parametrize("tangent", [False, True], ids=["secant", "tangent"])
@pytest.mark.parametrize("device_entry", [False, True], ids=["host", "device"])
def test_abi_argument_checks(lib, device_entry, tangent):
    buf, buf2 = np.zeros(64), np.zeros(64)
    p, p2 = buf.ctypes.data, buf2.ctypes.data
    fn = getattr(lib, NAMES[2 * tangent + device_entry])
    tail = (None,) if device_entry else ()
    keep = []
    fake = _fake_plan(2, _lib.KIND_ELASTICITY_ISO)  # t = 3, n_comp = 2; its tangent kind is Voigt
    plan = ctypes.addressof(fake)
    sibling = _fake_plan(2, _lib.KIND_ELASTICITY_VOIGT)
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))

    def secant(prog=None, **kw):
        prog = prog or _program(HIST, n_comp=4)
        keep.append((prog, prog.struct()))
        base = dict(program=ctypes.pointer(keep[-1][1]), n_fields=0, rows=p, points=p, xi=p, max_iter=5, tol=1e-10, relax=1.0, state=p, A_eff=p)
        keep.append(_lib.SecantArgs(**dict(base, **kw)))
        return keep[-1]

    def args(s=None, **kw):
        s = s if s is not None else secant()
        if not tangent:
            assert not kw
            return s
        base = dict(secant=ctypes.pointer(s), tangent_plan=ctypes.addressof(sibling), tangent=p, asymmetry=p)
        return _lib.SecantTangentArgs(**dict(base, **kw))

    def hist(n=2, i=p, o=p2):
        return _lib.HistoryArgs(n, i, o)

    def call(pl, src, a, h, n_cells=1):
        rc = fn(pl, n_cells, src, None, None if a is None else ctypes.byref(a), None if h is None else ctypes.byref(h), *tail)
        return rc, lib.hommx_last_error().decode()

    def refused(a, text, h=None, src=sampled):
        rc, msg = call(plan, src, a, hist() if h is None else h)
        assert rc == -1 and text in msg, (text, msg)

    # what opens every entry of the family
    rc, msg = call(None, sampled, args(), hist())
    assert rc == -1 and "null plan" in msg
    assert call(plan, None, None, None, n_cells=0)[0] == 0  # an empty batch reads nothing
    assert call(plan, sampled, args(), hist(), n_cells=-1)[0] == -1
    refused(args(), "null source", src=None)
    rc, msg = call(plan, sampled, None, hist())
    assert rc == -1 and msg == "null arguments"
    # the history struct
    rc, msg = call(plan, sampled, args(), None)
    assert rc == -1 and "null history arguments" in msg
    for n in (0, -1, 5):
        refused(args(), f"n_history must be 1 .. 4, got {n}", hist(n))
    refused(args(), "null history_in / history_out", hist(i=None))
    refused(args(), "null history_in / history_out", hist(o=None))
    refused(args(), "history_in and history_out are the same array", hist(o=p))
    # everything the entries without history refuse, through the same checks
    refused(args(secant(program=None)), "null program")
    for name in ("rows", "xi", "state", "A_eff"):
        refused(args(secant(**{name: None})), "null rows / xi / state / A_eff")
    refused(args(secant(strain=p)), "strain and flux: both or neither")
    refused(args(secant(n_fields=5)), "n_fields must be 0 .. 4, got 5")
    refused(args(secant(max_iter=0)), "max_iter must be at least 1, got 0")
    refused(args(secant(tol=float("nan"))), "tol must be a number >= 0")
    refused(args(secant(relax=1.5)), "relax must lie in (0, 1]")
    # the program against n_comp + n_history components on a row of 3 + n_fields + 2 t + n_comp + n_history entries
    refused(args(secant(_program(BOTH))), "n_comp is 2, the plan's coefficient and the history have 4 components together")
    refused(args(), "n_comp is 4, the plan's coefficient and the history have 3 components together", hist(1))
    refused(args(secant(_program([(OP_X, 13), (OP_STORE, 0)] + HIST[2:], n_comp=4))),
            "x index 13 out of range [0,13) (the midpoint, 0 fields and the 2 t + n_comp + n_history = 10 state entries)")
    refused(args(secant(_program(HIST[:6], n_comp=4))), "component 3 never stored")
    refused(args(secant(_program(HIST[:6] + [(OP_X, 12), (OP_STORE, 2)], n_comp=4))), "component 2 stored twice")
    refused(args(secant(_program(HIST[:6] + [(OP_X, 12), (OP_STORE, 4)], n_comp=4))), "component index 4 out of range [0,4)")
    four = BOTH + [op for k in range(4) for op in ((OP_X, 11 + k), (OP_STORE, 2 + k))]  # the 25 flags: here 2 + 4 of them on a row of 15
    refused(args(secant(_program(four[:-2], n_comp=6))), "component 5 never stored", hist(4))
    refused(args(secant(_program([(OP_X, 15), (OP_STORE, 0)] + four[2:], n_comp=6))), "x index 15 out of range [0,15)", hist(4))
    if tangent:
        for name in ("tangent_plan", "tangent", "asymmetry"):
            refused(args(**{name: None}), "null tangent_plan / tangent / asymmetry")
        refused(args(tangent_plan=plan), "tangent_plan is the plan itself")
        # an s read anywhere in the program, the updates included: s[k] is X 6 + k on this plan
        refused(args(secant(_program([(OP_X, 7), (OP_STORE, 0)] + HIST[2:], n_comp=4))), "the law reads s[1] (instruction 0)")
        refused(args(secant(_program(HIST[:6] + [(OP_X, 8), (OP_STORE, 3)], n_comp=4))), "the law reads s[2] (instruction 6)")
    # a sound call passes every check up to the device, which plan-shaped memory cannot serve -- so ask for too much
    if device_entry:
        rc, msg = call(plan, sampled, args(), hist(), n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg
        rc, msg = call(plan, sampled, args(secant(_program(four, n_comp=6))), hist(4), n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg


def test_the_entries_without_history_still_refuse_a_history_program(lib):
    """hommx_secant_source checks against the plan's n_comp and the shorter row, as it did."""
    buf = np.zeros(64)
    p = buf.ctypes.data
    fake = _fake_plan(2, _lib.KIND_ELASTICITY_ISO)
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    prog = _program(HIST, n_comp=4)
    st = prog.struct()
    a = _lib.SecantArgs(program=ctypes.pointer(st), rows=p, points=p, xi=p, max_iter=1, tol=0.0, relax=1.0, state=p, A_eff=p)
    assert lib.hommx_secant_source(ctypes.addressof(fake), 1, sampled, None, ctypes.byref(a)) == -1
    assert "n_comp is 4, the plan's coefficient has 2 components" in lib.hommx_last_error().decode()
