"""The argument checks of hommx_secant_state_source[_device] on plan-shaped memory: every refusal runs before the plan's
device is made current, so none of them needs a GPU (the manner of tests/test_secant_load_abi_host.py)."""

import ctypes
import os

import numpy as np
import pytest

from hommx_amd import _lib
from hommx_amd.expr import OP_STORE, OP_X, OP_Y
from test_secant_abi_host import BOTH, _fake_plan, _program

NAMES = ("hommx_secant_state_source", "hommx_secant_state_source_device")


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
    assert "} hommx_secant_state_args;" in header


def test_struct_layout_matches_the_header():
    """hommx_secant_state_args as the C compiler lays it out: two int32 padded to 8 where a pointer or a double follows, two int32
    sharing eight bytes; the structs beside it are untouched."""
    f = {name: getattr(_lib.SecantStateArgs, name).offset for name, _ in _lib.SecantStateArgs._fields_}
    names = ("crit_program", "crit_n_fields", "crit_rows", "threshold", "crit", "crit_values", "total_strain", "total_flux", "reconstruct",
             "n_regions", "region", "stats", "region_stats")
    assert [n for n, _ in _lib.SecantStateArgs._fields_] == list(names)
    assert [f[n] for n in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 80, 88]
    assert ctypes.sizeof(_lib.SecantStateArgs) == 96
    assert ctypes.sizeof(_lib.SecantArgs) == 136 and ctypes.sizeof(_lib.HistoryArgs) == 24 and ctypes.sizeof(_lib.SecantLoadArgs) == 24


@pytest.mark.parametrize("device_entry", [False, True], ids=["host", "device"])
def test_abi_argument_checks(lib, device_entry):
    buf = np.zeros(64)
    p = buf.ctypes.data
    fn = getattr(lib, NAMES[device_entry])
    tail = (None,) if device_entry else ()
    keep = []
    fake = _fake_plan(2, _lib.KIND_ELASTICITY_ISO)  # t = 3, n_comp = 2: the state row has 3 + n_fields + 6 + 4 + n_history entries
    plan = ctypes.addressof(fake)
    sampled = ctypes.byref(_lib.CoefSource(form=_lib.COEF_SAMPLED, coef=p))
    per_cell = _lib.SecantLoadArgs(_lib.LOADS_PER_CELL, p, None)
    one = _lib.HistoryArgs(1, p, p + 8)

    def secant(prog=None, **kw):
        prog = prog or _program(BOTH)
        keep.append((prog, prog.struct()))
        base = dict(program=ctypes.pointer(keep[-1][1]), n_fields=0, rows=p, points=p, xi=p, max_iter=5, tol=1e-10, relax=1.0, state=p, A_eff=p)
        keep.append(_lib.SecantArgs(**dict(base, **kw)))
        return keep[-1]

    def history_law():  # lam = c[0], mu = c[1], the update h[0]: three stores on the row with one history entry
        return secant(_program(BOTH + [(OP_X, 11), (OP_STORE, 2)], n_comp=3))

    def state(ops=((OP_X, 6), (OP_STORE, 0)), n_comp=1, **kw):
        base = dict(crit_n_fields=0, crit_rows=p, threshold=1.0, crit=p)
        if ops is not None:
            prog = _program(list(ops), n_comp=n_comp)
            keep.append((prog, prog.struct()))
            base["crit_program"] = ctypes.pointer(keep[-1][1])
        keep.append(_lib.SecantStateArgs(**dict(base, **kw)))
        return keep[-1]

    def call(pl, src, a, hist, load, st, n_cells=1):
        ref = lambda x: None if x is None else ctypes.byref(x)
        rc = fn(pl, n_cells, src, None, ref(a), ref(hist), ref(load), ref(st), *tail)
        return rc, lib.hommx_last_error().decode()

    def refused(text, st=None, a=None, hist=None, load=None, src=sampled):
        rc, msg = call(plan, src, a if a is not None else (history_law() if hist is not None else secant()), hist, load,
                       st if st is not None else state())
        assert rc == -1 and text in msg, (text, msg)

    def passes_the_checks(st, hist=None, load=None):
        """Plan-shaped memory cannot serve a call: one that passes every check is asked for too much (the device entry's last check)."""
        if device_entry:
            rc, msg = call(plan, sampled, history_law() if hist is not None else secant(), hist, load, st, n_cells=2**31)
            assert rc == -1 and "too large for one launch" in msg, msg

    # what opens every entry of the family
    rc, msg = call(None, sampled, secant(), None, None, state())
    assert rc == -1 and "null plan" in msg
    assert call(plan, None, None, None, None, None, n_cells=0)[0] == 0  # an empty batch reads nothing
    assert call(plan, sampled, secant(), None, None, state(), n_cells=-1)[0] == -1
    refused("null source", src=None)
    rc, msg = call(plan, sampled, None, None, None, state())
    assert rc == -1 and msg == "null arguments"
    # everything the underlying entries refuse, through the same checks
    refused("null program", a=secant(program=None))
    refused("null rows / xi / state / A_eff", a=secant(state=None))
    refused("strain and flux: both or neither", a=secant(strain=p))
    refused("max_iter must be at least 1, got 0", a=secant(max_iter=0))
    refused("n_history must be 1 .. 4, got 0", hist=_lib.HistoryArgs(0, p, p + 8))
    refused("history_in and history_out are the same array", hist=_lib.HistoryArgs(1, p, p))
    refused("unknown load code 7 in per_cell", load=_lib.SecantLoadArgs(7, p, None))
    refused("null P", load=_lib.SecantLoadArgs(_lib.LOADS_PER_CELL, None, None))
    # the state struct
    rc, msg = call(plan, sampled, secant(), None, None, None)
    assert rc == -1 and msg == "null state arguments"
    refused("nothing requested: neither a criterion nor the reconstruction", state(ops=None))
    # ... its criterion, as hommx_criterion_source checks one
    refused("null crit_rows / crit", state(crit_rows=None))
    refused("null crit_rows / crit", state(crit=None))
    refused("total_strain and total_flux: both or neither", state(total_strain=p))
    refused("total_strain and total_flux: both or neither", state(total_flux=p))
    refused("n_fields must be 0 .. 4, got 5", state(crit_n_fields=5))
    refused("n_comp is 2, a criterion has one component", state(ops=BOTH, n_comp=2))
    refused("the threshold is NaN", state(threshold=float("nan")))
    refused("null points: the criterion reads y (instruction 0)", state(ops=[(OP_Y, 0), (OP_STORE, 0)]), a=secant(points=None))
    # the row: [x 0..2 | e 3..5 | s 6..8 | c 9..10 | h (n_history) | b (2)]
    passes_the_checks(state(ops=[(OP_X, 12), (OP_STORE, 0)]))  # b[1] without a history
    refused("x index 13 out of range [0,13)", state(ops=[(OP_X, 13), (OP_STORE, 0)]))  # an index of the h segment needs a history struct
    passes_the_checks(state(ops=[(OP_X, 13), (OP_STORE, 0)]), hist=one)  # b[1] behind one history entry
    refused("x index 14 out of range [0,14)", state(ops=[(OP_X, 14), (OP_STORE, 0)]), hist=one)
    refused("x index 14 out of range [0,14)", state(ops=[(OP_X, 14), (OP_STORE, 0)]), hist=one, load=per_cell)
    # ... its reconstruction, as hommx_reconstruct_source checks one
    refused("null stats", state(ops=None, reconstruct=1))
    refused("n_regions must be 0 .. 8, got 9", state(ops=None, reconstruct=1, stats=p, n_regions=9))
    refused("region and region_stats: both with n_regions > 0", state(ops=None, reconstruct=1, stats=p, n_regions=2, region=p))
    refused("region and region_stats: both with n_regions > 0", state(ops=None, reconstruct=1, stats=p, n_regions=2, region_stats=p))
    refused("region and region_stats: both with n_regions > 0", state(ops=None, reconstruct=1, stats=p, n_regions=0, region=p))
    refused("reconstruct together with a load", state(ops=None, reconstruct=1, stats=p), load=per_cell)
    refused("reconstruct together with a load", state(reconstruct=1, stats=p), load=per_cell, hist=one)
    passes_the_checks(state(reconstruct=1, stats=p, n_regions=2, region=p, region_stats=p, crit_values=p, total_strain=p, total_flux=p), hist=one)
    passes_the_checks(state(crit_values=p), load=per_cell)
