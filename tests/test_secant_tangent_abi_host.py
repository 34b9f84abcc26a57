"""The argument checks of hommx_secant_tangent_source[_device] on plan-shaped memory: every refusal runs before the plan's device is
made current, so none of them needs a GPU (the manner of tests/test_secant_abi_host.py)."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib
from hommx_amd.batch import Program
from hommx_amd.expr import OP_STORE, OP_X, SecantLaw
from test_secant_abi_host import BOTH, _fake_plan, _program


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_the_symbols_are_exported(lib):
    names = ("hommx_secant_tangent_source", "hommx_secant_tangent_source_device")
    assert set(names) <= set(_lib.EXPORTED_SYMBOLS)
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hommx_hip.h")).read()
    for name in names:
        assert getattr(lib, name) is not None and f"int {name}(" in header
    assert "} hommx_secant_tangent_args;" in header


@pytest.mark.parametrize("device_entry", [False, True])
def test_abi_argument_checks(lib, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = lib.hommx_secant_tangent_source_device if device_entry else lib.hommx_secant_tangent_source
    tail = (None,) if device_entry else ()
    keep = []
    fake = _fake_plan(2, _lib.KIND_ELASTICITY_ISO)  # t = 3, n_comp = 2: a row of 3 + n_fields + 8 entries; its tangent kind is Voigt
    plan = ctypes.addressof(fake)
    sibling = _fake_plan(2, _lib.KIND_ELASTICITY_VOIGT)
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))

    def call(pl, src, args, n_cells=1):
        rc = fn(pl, n_cells, src, None, None if args is None else ctypes.byref(args), *tail)
        return rc, lib.hommx_last_error().decode()

    def secant(prog=None, **kw):
        prog = prog or _program(BOTH)
        keep.append((prog, prog.struct()))
        base = dict(program=ctypes.pointer(keep[-1][1]), n_fields=0, rows=p, points=p, xi=p, max_iter=5, tol=1e-10, relax=1.0, state=p, A_eff=p)
        keep.append(_lib.SecantArgs(**dict(base, **kw)))
        return ctypes.pointer(keep[-1])

    def args(s=None, **kw):
        base = dict(secant=s or secant(), tangent_plan=ctypes.addressof(sibling), tangent=p, asymmetry=p)
        return _lib.SecantTangentArgs(**dict(base, **kw))

    def refused(a, text, src=sampled):
        rc, msg = call(plan, src, a)
        assert rc == -1 and text in msg, (text, msg)

    # what opens every entry of the family
    rc, msg = call(None, sampled, args())
    assert rc == -1 and "null plan" in msg
    assert call(plan, None, None, n_cells=0)[0] == 0  # an empty batch reads nothing
    assert call(plan, sampled, args(), n_cells=-1)[0] == -1
    refused(args(), "null source", None)
    refused(args(), "unknown coefficient form 7", ctypes.byref(_lib.CoefSource(form=7, coef=p)))
    rc, msg = call(plan, sampled, None)
    assert rc == -1 and msg == "null arguments"
    refused(_lib.SecantTangentArgs(tangent_plan=ctypes.addressof(sibling), tangent=p, asymmetry=p), "null secant arguments")
    # everything hommx_secant_source refuses, through the same checks
    refused(args(secant(program=None)), "null program")
    for name in ("rows", "xi", "state", "A_eff"):
        refused(args(secant(**{name: None})), "null rows / xi / state / A_eff")
    refused(args(secant(strain=p)), "strain and flux: both or neither")
    refused(args(secant(n_fields=5)), "n_fields must be 0 .. 4, got 5")
    refused(args(secant(_program([(OP_X, 0), (OP_STORE, 0)], n_comp=1))), "n_comp is 1, the plan's coefficient has 2 components")
    refused(args(secant(_program([(OP_X, 11), (OP_STORE, 0)] + BOTH[2:]))), "x index 11 out of range [0,11)")
    refused(args(secant(_program(BOTH[:2]))), "component 1 never stored")
    refused(args(secant(max_iter=0)), "max_iter must be at least 1, got 0")
    refused(args(secant(tol=float("nan"))), "tol must be a number >= 0")
    refused(args(secant(relax=1.5)), "relax must lie in (0, 1]")
    # the tangent's own arguments
    for name in ("tangent_plan", "tangent", "asymmetry"):
        refused(args(**{name: None}), "null tangent_plan / tangent / asymmetry")
    refused(args(tangent_plan=plan), "tangent_plan is the plan itself")
    for kind in (_lib.KIND_POISSON_SCALAR, _lib.KIND_POISSON_MATRIX, _lib.KIND_ELASTICITY_ISO):
        other = _fake_plan(2, kind)
        refused(args(tangent_plan=ctypes.addressof(other)), f"tangent_plan has kind {kind}; the tangent kind of a plan of kind 2 is 3")
    other = _fake_plan(3, _lib.KIND_ELASTICITY_VOIGT)
    refused(args(tangent_plan=ctypes.addressof(other)), "tangent_plan has dim 3; the plan has 2")
    other = ctypes.create_string_buffer(4096)
    ctypes.memmove(other, ctypes.byref(_lib.PlanDesc(2, 9, _lib.KIND_ELASTICITY_VOIGT, 0, 0)), ctypes.sizeof(_lib.PlanDesc))
    refused(args(tangent_plan=ctypes.addressof(other)), "tangent_plan has n_micro 9; the plan has 8")
    ctypes.memmove(other, ctypes.byref(_lib.PlanDesc(2, 8, _lib.KIND_ELASTICITY_VOIGT, 1, 0)), ctypes.sizeof(_lib.PlanDesc))
    refused(args(tangent_plan=ctypes.addressof(other)), "tangent_plan is on device 1; the plan on 0")
    # an implicit law: s[k] is X 6 + k on this plan (the midpoint, no field, e of t = 3)
    for k in range(3):
        refused(args(secant(_program([(OP_X, 6 + k), (OP_STORE, 0)] + BOTH[2:]))), f"the law reads s[{k}] (instruction 0)")
    refused(args(secant(_program([(OP_X, 8 + 2), (OP_STORE, 0)] + BOTH[2:]), n_fields=2)), "the law reads s[2] (instruction 0)")
    # e and c are not s: such a law passes every check up to the device, which plan-shaped memory cannot serve -- so ask for too much
    if device_entry:
        ok = args(secant(_program([(OP_X, 5), (OP_STORE, 0)] + BOTH[2:])))
        rc, msg = call(plan, sampled, ok, n_cells=2**31)
        assert rc == -1 and "too large for one launch" in msg


def test_a_mesh_plan_takes_a_sibling_of_its_own_mesh(lib):
    """The descriptor of a mesh plan (n_micro == 0) holds no size, so the element count behind it is compared (and, of real plans with
    equal counts, the nodes).  Plan-shaped memory: `int64_t n_el` follows the descriptor (32 bytes) and the family (an int, padded to 8), at byte 40."""
    buf = np.zeros(8)
    p = buf.ctypes.data
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))

    def mesh_shaped(kind, n_el):
        fake = ctypes.create_string_buffer(4096)
        ctypes.memmove(fake, ctypes.byref(_lib.PlanDesc(2, 0, kind, 0, 0)), ctypes.sizeof(_lib.PlanDesc))
        ctypes.memmove(ctypes.addressof(fake) + ctypes.sizeof(_lib.PlanDesc) + 8, ctypes.byref(ctypes.c_int64(n_el)), 8)
        return fake

    assert ctypes.sizeof(_lib.PlanDesc) == 32
    prog = _program(BOTH)
    st = prog.struct()
    s = _lib.SecantArgs(program=ctypes.pointer(st), rows=p, points=p, xi=p, max_iter=1, tol=0.0, relax=1.0, state=p, A_eff=p)
    plan, other = mesh_shaped(_lib.KIND_ELASTICITY_ISO, 126), mesh_shaped(_lib.KIND_ELASTICITY_VOIGT, 112)
    a = _lib.SecantTangentArgs(secant=ctypes.pointer(s), tangent_plan=ctypes.addressof(other), tangent=p, asymmetry=p)
    for fn, tail in ((lib.hommx_secant_tangent_source, ()), (lib.hommx_secant_tangent_source_device, (None,))):
        assert fn(ctypes.addressof(plan), 1, sampled, None, ctypes.byref(a), *tail) == -1
        assert "tangent_plan is a plan of another mesh: 112 elements, the plan has 126" in lib.hommx_last_error().decode()


def test_the_poisson_kinds_take_the_matrix_kind(lib):
    buf = np.zeros(8)
    p = buf.ctypes.data
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    ops, consts = SecantLaw("c[0]*e[1]").program(2, 1)
    prog = Program(ops, consts, 1)
    st = prog.struct()
    s = _lib.SecantArgs(program=ctypes.pointer(st), rows=p, points=p, xi=p, max_iter=1, tol=0.0, relax=1.0, state=p, A_eff=p)
    for kind, text in ((_lib.KIND_POISSON_SCALAR, "kind 0; the tangent kind of a plan of kind 0 is 1"),
                       (_lib.KIND_ELASTICITY_VOIGT, "kind 3; the tangent kind of a plan of kind 0 is 1")):
        fake, other = _fake_plan(2, _lib.KIND_POISSON_SCALAR), _fake_plan(2, kind)
        a = _lib.SecantTangentArgs(secant=ctypes.pointer(s), tangent_plan=ctypes.addressof(other), tangent=p, asymmetry=p)
        assert lib.hommx_secant_tangent_source(ctypes.addressof(fake), 1, sampled, None, ctypes.byref(a)) == -1
        assert text in lib.hommx_last_error().decode()


def test_struct_layout_matches_the_header():
    """hommx_secant_tangent_args as the C compiler lays it out: six pointers."""
    f = {name: getattr(_lib.SecantTangentArgs, name).offset for name, _ in _lib.SecantTangentArgs._fields_}
    assert [f[n] for n in ("secant", "tangent_plan", "tangent", "asymmetry", "tangent_coef", "tangent_info")] == [0, 8, 16, 24, 32, 40]
    assert ctypes.sizeof(_lib.SecantTangentArgs) == 48
    assert ctypes.sizeof(_lib.SecantArgs) == 136  # hommx_secant_args is untouched
