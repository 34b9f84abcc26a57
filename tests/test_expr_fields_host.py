"""Fields ``f[k]`` of an ``Expression`` on the CPU: the grammar and what it emits (``X 3 + k``), the degrees and names, the rows the host
paths take (the fields ride as extra rows of ``x``), the tangent rules of ``host_tangents`` with a field as the argument against the
closed-form derivatives of test_expr_params_host.py, the equivalence of a field that has one value in every cell with a parameter, the
validation of ``n_fields`` and of the differentiable slots at the C ABI (on the host, before the plan's device is made current) and
``set_fields`` / ``cell_means`` of the solver classes on oracle-backed stand-in plans.  Field values differ from cell to cell wherever
cells are compared.  No GPU needed."""

import ctypes as C
import logging

import numpy as np
import pytest

from hommx_amd import _lib, expr, hmm, mesh
from hommx_amd.batch import CoefStream, Program
from hommx_amd.expr import Expression as E
from test_expr_params_host import EXACT, ROUNDED, _dyadic_case, _sens_call, lib  # noqa: F401  (lib: the fixture)
from test_hmm_host import with_oracle
from test_program_abi_host import GOOD, P as PTR, call, source
from test_reconstruct_source_host import _fake_plan


def _as_fields(text):
    """The text with every parameter read as the field of the same index."""
    return text.replace("p[", "f[")


# -- 1. grammar and emission -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,kw,message", [
    ("1 + f[0]", {}, "only x and y are indexed: Subscript 'f[0]'"),
    ("1 + f[0]", dict(p=[1.0]), "only x and y are indexed: Subscript 'f[0]'"),
    ("1 + f[1]", dict(fields=1), "the index of f is a literal integer below the number of fields (1): Subscript 'f[1]'"),
    ("1 + f[-1]", dict(fields=1), "the index of f is a literal integer below the number of fields (1): Subscript 'f[-1]'"),
    ("1 + f[x[0]]", dict(fields=2), "the index of f is a literal integer below the number of fields (2): Subscript 'f[x[0]]'"),
    ("1 + f[0]", dict(fields=5), "at most 4 fields; got 5"),
    ("1 + f[0]", dict(fields=("a", "b", "c", "d", "e")), "at most 4 fields; got 5"),
    ("1 + f[0]", dict(fields=-1), "fields must be a count 0 .. 4 or a sequence of names"),
    ("1 + f[0]", dict(fields=1.5), "fields must be a count 0 .. 4 or a sequence of names"),
    ("1 + f", dict(fields=1), "unknown name"),
])
def test_errors_name_the_fault(text, kw, message):
    with pytest.raises(ValueError) as e:
        E(text, **kw)
    assert str(e.value).startswith("expression: ") and message in str(e.value)


def test_a_field_is_an_x_instruction_past_the_midpoint():
    A = E("2*f[1] + x[2]*f[0] + p[0]", p=[0.5], fields=("radius", "phase"))
    ops, consts = A.program()
    X, K, MUL, ADD, ST = expr.OP_X, expr.OP_CONST, expr.OP_MUL, expr.OP_ADD, expr.OP_STORE
    assert ops.tolist() == [[K, 1], [X, 4], [MUL, 0], [X, 2], [X, 3], [MUL, 0], [ADD, 0], [K, 0], [ADD, 0], [ST, 0]]
    assert consts.tolist() == [0.5, 2.0]  # a field takes no constant
    assert (A.n_fields, A.field_names, A.n_params, A.parameter_names) == (2, ("radius", "phase"), 1, ("p0",))
    assert E("f[0]", fields=1).field_names == ("f0",) and E("f[3]", fields=4).program()[0].tolist() == [[X, 6], [ST, 0]]
    assert E("y[0]").n_fields == 0 and E("y[0]").field_names == () and E("y[0]", fields=0).n_fields == 0
    assert E("y[0]", fields=3).n_fields == 3  # admitted, not read: the row still carries them
    assert expr.MAX_FIELDS == _lib.PROGRAM_MAX_FIELDS == 4
    B = A.with_parameters([2.0])  # the parameters change, the fields stay admitted
    assert (B.n_fields, B.field_names) == (2, ("radius", "phase")) and np.array_equal(B.program()[0], ops)
    M = E([["1 + f[0]", "f[1]*y[0]"], ["f[1]*y[0]", "2"]], fields=2)  # the symmetry check reads fields too
    assert M.n_comp == 3 and M.n_fields == 2
    with pytest.raises(ValueError, match="must be symmetric"):
        E([["1", "f[0]"], ["f[1]", "2"]], fields=2)


@pytest.mark.parametrize("text,degree,p_degree", [
    ("f[0]", 0, 1), ("f[0]*y[0]", 1, 1), ("f[0]*f[1]", 0, 2), ("p[0]*f[0]", 0, 2), ("p[0] + f[1]*sin(2*pi*y[0])", 3, 1),
    ("(f[0] + y[0])**3", 3, 3), ("y[1]/(1 + f[0])", 1, np.inf), ("tanh(f[0]*(y[0] - 0.5))", 3, np.inf), ("abs(f[0])", 0, np.inf),
    ("where(y[0] < 0.5, f[1], 2*f[0])", 0, 1), ("x[0] + y[0]", 1, 0),
])
def test_degrees_count_fields_with_parameters(text, degree, p_degree, caplog):
    with caplog.at_level(logging.WARNING):
        A = E(text, p=[0.5], fields=2)
    assert (A.degree, A.p_degree, A.affine_in_parameters) == (degree, p_degree, p_degree <= 1)
    assert not caplog.records


def test_a_field_inside_a_comparison_warns_once(caplog):
    with caplog.at_level(logging.WARNING):
        A = E([["where(y[0] < f[0], 2, 1)", "0"], ["0", "where(y[1] < f[0] or y[0] > p[0], 2, 1)"]], p=[0.5], fields=1)
    assert A.p_degree == 0 and A.affine_in_parameters
    warnings = [r for r in caplog.records if r.levelname == "WARNING"]
    assert len(warnings) == 1 and "inside a comparison" in warnings[0].getMessage() and "y[0] < f[0]" in warnings[0].getMessage()
    x = np.array([[0.0, 0.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.875]])
    yq = np.array([[[0.25, 0.5]], [[0.75, 0.5]]])
    assert A.host_stream(x, yq, np.ones(1))[:, :, 0].tolist() == [[2.0, 1.0], [2.0, 2.0]]  # the interface sits where the cell puts it
    assert not A.host_tangents(x, yq, np.ones(1)).any()


# -- 2. the rows -------------------------------------------------------------------------------------------------------------------------
def test_every_host_path_takes_the_extended_x_and_names_the_fields_when_given_less():
    A = E("1 + f[0]*y[0] + f[1]", fields=("radius", "phase"))
    x, yq, w = np.array([[0.0, 0.0, 0.0, 2.0, 0.5], [0.0, 0.0, 0.0, 4.0, 0.25]]), np.array([[[0.5, 0.0]], [[0.25, 0.0]]]), np.ones(1)
    assert A.host_stream(x, yq, w).tolist() == [[2.5, 2.0], [3.25, 2.25]]
    assert A.host_tangents(x, yq, w).tolist() == [[[0.5, 0.25], [1.0, 1.0]]] * 2
    assert A(x[1], yq[:, 0].T).tolist() == [3.25, 2.25]  # the plain callable of the generic paths: x[3 + n_fields], y[d, npts]
    assert A(x.T[:, :, None], yq[:, 0].T[:, None, :]).tolist() == [[2.5, 2.0], [3.25, 2.25]]
    for call_ in (lambda: A.host_stream(x[:, :4], yq, w), lambda: A.host_tangents(x[:, :3], yq, w), lambda: A(x[0, :3], yq[:, 0].T),
                  lambda: A.components(x.T[:4, :, None], yq[:, 0].T[:, None, :])):
        with pytest.raises(ValueError, match=r"reads the fields radius, phase: x must have 3 \+ 2 entries"):
            call_()
    plain = E("1 + x[0]*y[0]")  # without fields nothing changes: three entries, as ever
    assert plain.host_stream(x[:, :3], yq, w).shape == (2, 2) and plain(x[0, :3], yq[:, 0].T).shape == (2,)


# -- 3. the rules with a field as the argument -------------------------------------------------------------------------------------------
def _field_rows(x, n_fields, seed=3):
    """The midpoints with dyadic field values after them, different in every cell."""
    rng = np.random.default_rng(seed)
    v = (4 + np.arange(len(x))[:, None] * n_fields + np.arange(n_fields)[None, :] + rng.integers(0, 2, (len(x), n_fields))) / 8.0
    assert len(np.unique(v)) > len(x)
    return np.concatenate([x, v], axis=1)


@pytest.mark.parametrize("text,derivatives,condition", EXACT, ids=[c[0] for c in EXACT])
def test_exact_rules_equal_the_closed_form_bitwise(text, derivatives, condition):
    x, yq, w = _dyadic_case()
    rows = _field_rows(x, 2)
    got = E(_as_fields(text), fields=2).host_tangents(rows, yq, w)
    assert got.shape == (5, 2, 11) and np.all(np.isfinite(got))
    for j, d in enumerate(derivatives):
        want = np.broadcast_to(E(_as_fields(d), fields=2).host_stream(rows, yq, w), (5, 11))
        assert np.array_equal(got[:, j], want), (j, d)
    assert len({rows[c, 3:].tobytes() for c in range(5)}) == 5  # the cells differ: a field is no shared constant


@pytest.mark.parametrize("name,text,derivative", ROUNDED, ids=[c[0] for c in ROUNDED])
def test_rounded_rules_equal_the_closed_form_bitwise(name, text, derivative):
    rng = np.random.default_rng(11)
    x, yq = rng.uniform(0.0, 1.0, (4, 3)), rng.uniform(0.0, 1.0, (9, 1, 2))
    rows = np.concatenate([x, rng.uniform(0.4, 0.9, (4, 1))], axis=1)
    w = np.ones(1)
    got = E(_as_fields(text), fields=1).host_tangents(rows, yq, w)[:, 0]
    want = E(_as_fields(derivative), fields=1).host_stream(rows, yq, w)
    assert np.all(np.isfinite(want)) and np.abs(want).max() > 0.1
    assert np.array_equal(got, want)
    h = 2.0**-20  # and the closed form is the derivative with respect to the cell's own value: a central difference
    up, dn = rows.copy(), rows.copy()
    up[:, 3] += h
    dn[:, 3] -= h
    fd = (E(_as_fields(text), fields=1).host_stream(up, yq, w) - E(_as_fields(text), fields=1).host_stream(dn, yq, w)) / (2 * h)
    assert np.abs(fd - got).max() < 1e-8 * max(1.0, np.abs(got).max())


# -- 4. a field with one value in every cell is a parameter ------------------------------------------------------------------------------
TEXTS = ["1.1 + x[0] + p[0]*sin(2*pi*y[0]) + y[1]*(1 - y[1])/p[0]", "where(y[0] < 0.5, p[0]*y[1], sqrt(1 + p[0]*x[1])) + (p[0] + y[0])**3",
         "exp(p[0]*y[0])*tanh(x[2] - p[0]) + abs(p[0] - 2*y[1]) + min(p[0], y[0]) + max(y[1], p[0]*x[0])"]


@pytest.mark.parametrize("text", TEXTS)
def test_equal_field_values_give_the_stream_and_tangents_of_the_parameter_bitwise(text):
    rng = np.random.default_rng(17)
    x, yq, w = rng.uniform(0.0, 1.0, (6, 3)), rng.uniform(0.0, 1.0, (10, 3, 2)), np.array([0.2, 0.5, 0.3])
    v = 0.6180339887
    par, fld = E(text, p=[v]), E(_as_fields(text), fields=1)
    rows = np.concatenate([x, np.full((6, 1), v)], axis=1)
    assert np.array_equal(fld.host_stream(rows, yq, w), par.host_stream(x, yq, w))
    assert np.array_equal(fld.host_tangents(rows, yq, w), par.host_tangents(x, yq, w))
    assert fld.degree == par.degree and fld.p_degree == par.p_degree


def test_the_slots_are_the_parameters_then_the_fields():
    rng = np.random.default_rng(19)
    x, yq, w = rng.uniform(0.0, 1.0, (5, 3)), rng.uniform(0.0, 1.0, (8, 2, 2)), np.array([0.25, 0.75])
    v = rng.uniform(0.5, 1.5, (5, 2))
    rows = np.concatenate([x, v], axis=1)
    A = E("p[1]*y[0] + f[0]*y[1] + p[0]*f[1]*x[0]", p=[0.5, 2.0], fields=2)
    got = A.host_tangents(rows, yq, w)
    assert got.shape == (5, 4, 8)
    want = ["f[1]*x[0]", "y[0]", "y[1]", "p[0]*x[0]"]  # d/dp0, d/dp1, d/df0, d/df1
    for j, d in enumerate(want):
        ref = np.broadcast_to(E(d, p=[0.5, 2.0], fields=2).host_stream(rows, yq, w), (5, 8))
        assert np.allclose(got[:, j], ref, rtol=4e-16, atol=0), (j, d)  # a sum of two roundings behind each
    # the same through the rules alone: every field made a parameter, cell by cell, fills the same slots with the same bits
    for c in range(5):
        B = E("p[1]*y[0] + p[2]*y[1] + p[0]*p[3]*x[0]", p=[0.5, 2.0, v[c, 0], v[c, 1]])
        assert np.array_equal(B.host_tangents(x[c:c + 1], yq, w)[0], got[c])
    with pytest.raises(ValueError, match="no parameters"):
        E("y[0]", fields=0).host_tangents(x, yq, w)


# -- 5. the ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_source_carries_n_fields_where_reserved_was():
    A = E("1 + f[1]*y[0] + p[0]", p=[0.5], fields=2)
    stream = CoefStream.program(np.zeros((2, 1, 2)), np.ones(1), *A.program(), A.n_comp, np.zeros((3, 5)), n_params=1, n_fields=2)
    prog = stream.shared[2]
    assert isinstance(prog, Program) and (prog.n_params, prog.n_fields) == (1, 2) and stream.per_cell.shape == (3, 5)
    src = stream.coef_source()
    assert src.n_fields == 2 and src.program.contents.n_params == 1
    assert CoefStream.program(np.zeros((2, 1, 2)), np.ones(1), *A.program(), A.n_comp, np.zeros((3, 3))).coef_source().n_fields == 0
    S = _lib.CoefSource
    assert S.n_fields.offset == 12 and S.n_fields.size == 4 and C.sizeof(S) == 72  # no struct grows
    assert C.sizeof(_lib.CoefProgram) == 32
    import os

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hommx_hip.h")).read()
    assert "#define HOMMX_PROGRAM_MAX_FIELDS 4" in hdr and "int32_t n_fields;" in hdr


F0 = [(expr.OP_X, 3), (expr.OP_STORE, 0)]  # the program "f[0]"
ENTRIES = {"hommx_solve_batch_source": (None, PTR, None), "hommx_expand_source": (PTR,), "hommx_expand_source_device": (PTR, None),
           "hommx_expand_tangents": (PTR, PTR), "hommx_expand_tangents_device": (PTR, PTR, None)}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_n_fields_and_the_x_index_are_validated_on_every_path(lib, entry):
    plan = C.addressof(_fake_plan(_lib.KIND_POISSON_SCALAR))
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan = C.addressof(fake)
    for bad in (-1, 5):
        rc, msg = call(lib, entry, plan, 1, source(ops=GOOD, n_fields=bad), ENTRIES[entry])
        assert rc == -1 and f"n_fields must be 0 .. 4, got {bad}" in msg, (rc, msg)
    rc, msg = call(lib, entry, plan, 1, source(ops=[(expr.OP_X, 5), (expr.OP_STORE, 0)], n_fields=2), ENTRIES[entry])
    assert rc == -1 and "x index 5 out of range [0,5)" in msg and "2 fields" in msg, (rc, msg)
    rc, msg = call(lib, entry, plan, 1, source(ops=F0), ENTRIES[entry])  # without fields: today's text, byte for byte
    assert rc == -1 and msg == "program: x index 3 out of range [0,3) at instruction 0", (rc, msg)
    if "tangents" not in entry:  # a field index inside the row passes: the call gets as far as its own pointer check
        rc, msg = call(lib, entry, plan, 1, source(ops=[(expr.OP_X, 6), (expr.OP_STORE, 0)], n_fields=4), tuple(None for _ in ENTRIES[entry]))
        assert rc == -1 and msg.startswith("null "), (rc, msg)


def test_n_fields_is_read_for_the_program_form_only(lib):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    src = _lib.CoefSource(form=_lib.COEF_SAMPLED, n_fields=77)  # whatever a caller left in the word that was reserved
    rc, msg = call(lib, "hommx_solve_batch_source", C.addressof(fake), 1, C.byref(src), (None, PTR, None))
    assert rc == -1 and msg == "null coef"


@pytest.mark.parametrize("entry", ["hommx_expand_tangents", "hommx_expand_tangents_device"])
def test_expand_tangents_counts_parameters_and_fields(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan, tail = C.addressof(fake), (None,) if entry.endswith("_device") else ()
    rc, msg = call(lib, entry, plan, 1, source(ops=F0, n_fields=1), (PTR, None) + tail)  # one field and no parameter is differentiable
    assert rc == -1 and msg == "null dirs_out", (rc, msg)
    rc, msg = call(lib, entry, plan, 1, source(ops=GOOD), (PTR, PTR) + tail)  # neither: today's text
    assert rc == -1 and "the program has no parameters (n_params == 0)" in msg, (rc, msg)
    for n_params, n_fields in ((1, 4), (4, 1), (2, 3)):
        kw = dict(ops=F0, consts=[1.0] * n_params, prog_n_params=n_params, n_fields=n_fields)
        rc, msg = call(lib, entry, plan, 1, source(**kw), (PTR, PTR) + tail)
        assert rc == -1 and f"at most 4 differentiable slots, got n_params ({n_params}) + n_fields ({n_fields}) = 5" in msg, (rc, msg)
    rc, msg = call(lib, entry, plan, 1, source(ops=F0, consts=[1.0] * 2, prog_n_params=2, n_fields=2), (PTR, None) + tail)
    assert rc == -1 and msg == "null dirs_out", (rc, msg)  # four together pass


@pytest.mark.parametrize("entry", ["hommx_sensitivity_source", "hommx_sensitivity_source_device", "hommx_second_sensitivity_source",
                                   "hommx_second_sensitivity_source_device"])
def test_parameter_directions_count_parameters_and_fields(lib, entry):
    fake = _fake_plan(_lib.KIND_POISSON_SCALAR)
    plan = C.addressof(fake)
    par = _lib.DIRS_PARAMETERS

    def args(n_dirs, dirs=None):
        return _lib.Sens2Args(n_dirs, par, dirs, PTR, None) if "second" in entry else _lib.SensArgs(n_dirs, par, dirs, PTR, None, None, None, None)

    mixed = dict(ops=F0, consts=[1.0, 2.0], prog_n_params=2, n_fields=1)
    for n_dirs in (2, 1, 4):  # n_params alone, n_fields alone, something else
        rc, msg = _sens_call(lib, entry, plan, source(**mixed), args(n_dirs))
        assert rc == -1 and f"n_dirs must be the source's n_params (2) + n_fields (1), got {n_dirs}" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(**mixed), args(3, PTR))
    assert rc == -1 and "dirs must be NULL" in msg, (rc, msg)  # n_dirs == n_tan passes the count
    rc, msg = _sens_call(lib, entry, plan, source(ops=F0, consts=[1.0] * 3, prog_n_params=3, n_fields=2), args(5))
    assert rc == -1 and "at most 4 differentiable slots, got n_params (3) + n_fields (2) = 5" in msg, (rc, msg)
    rc, msg = _sens_call(lib, entry, plan, source(ops=GOOD, consts=[1.0, 2.0], prog_n_params=2), args(1))  # without fields: today's text
    assert rc == -1 and "n_dirs must be the program's n_params (2), got 1" in msg, (rc, msg)


def test_the_plan_checks_the_rows_of_a_stream():
    from hommx_amd.batch import MicroCellPlan

    A = E("1 + f[1]*y[0]", fields=2)
    p = MicroCellPlan.__new__(MicroCellPlan)  # shapes only: no library call
    p.n_el, p.dim, p.n_comp = 2, 2, 1
    make = lambda rows: CoefStream.program(np.zeros((2, 1, 2)), np.ones(1), *A.program(), A.n_comp, np.zeros((3, rows)), n_fields=A.n_fields)
    assert p._check_stream(make(5)) == 3
    with pytest.raises(ValueError, match=r"midpoints has shape \(3, 3\); expected \(3, 3 \+ 2\): the midpoint, then the fields"):
        p._check_stream(make(3))
    assert MicroCellPlan._parameter_count(make(5)) == 2
    assert MicroCellPlan._parameter_count(CoefStream.program(np.zeros((2, 1, 2)), np.ones(1), *A.program(), 1, np.zeros((3, 5)), n_params=0,
                                                             n_fields=1)) == 1


# -- 6. the solver classes ---------------------------------------------------------------------------------------------------------------
TEXT = "1.1 + x[0] + f[0]*sin(2*pi*y[0]) + f[1]*y[1]*(1-y[1])"


def _solver(A=None, nx=3, n=4):
    msh = mesh.create_unit_square(nx, nx)
    h = hmm.PoissonHMM(msh, A or E(TEXT, fields=("amplitude", "bump")), lambda x: 1.0 + x[0], mesh.create_unit_square(n, n), 0.01)
    return with_oracle(h), msh


def _values(msh, seed=23):
    return np.random.default_rng(seed).uniform(0.1, 0.5, (msh.num_cells, 2))


def test_set_fields_shapes_values_and_the_error_before_it():
    h, msh = _solver()
    plan = h._plan
    for run in (h.solve, h.tensor_derivatives, lambda: h.reconstruct(np.zeros(h._num_global_dofs)), lambda: h._element_means(np.arange(2))):
        with pytest.raises(RuntimeError, match=r"reads the fields amplitude, bump: call set_fields\(\)"):
            run()
    v = _values(msh)
    for bad in (v[:-1], v[:, :1], v.T, v[:, 0], np.concatenate([v, v], axis=1)):
        with pytest.raises(ValueError, match=rf"need values of shape \({msh.num_cells}, 2\)"):
            h.set_fields(bad)
    for value in (np.nan, np.inf):
        w = v.copy()
        w[5, 1] = value
        with pytest.raises(ValueError, match="field bump is not finite on macro cell 5"):
            h.set_fields(w)
    assert h._fields is None
    h.set_fields(v)
    assert h._needs_reassembly and h._plan is plan
    h.solve()
    assert not h._needs_reassembly and h._plan is plan and not h.cell_info.any()
    first = h.effective_tensors.copy()
    v[4] += 0.125
    h.set_fields(v)  # the array is copied: changing the caller's does nothing
    v[7] = 9.0
    assert h._needs_reassembly and h._plan is plan
    h.solve()
    changed = np.any(h.effective_tensors != first, axis=(1, 2))
    assert changed.tolist() == [c == 4 for c in range(msh.num_cells)]  # a cell reads its own row and no other
    with pytest.raises(ValueError, match="set_fields"):
        _solver(E("1.1 + x[0]"))[0].set_fields(v)
    with pytest.raises(ValueError, match="set_fields"):
        _solver(lambda x, y: 1.0 + 0 * y[0])[0].set_fields(v)


def test_fields_reach_the_host_sampling_as_rows_of_x():
    h, msh = _solver()
    v = _values(msh)
    h.set_fields(v)
    cells = np.arange(msh.num_cells)
    got, kind = h._element_means(cells)
    plain = lambda c: (lambda x, y: 1.1 + x[0] + v[c, 0] * np.sin(2 * np.pi * y[0]) + v[c, 1] * y[1] * (1 - y[1]))
    g, _ = _solver(plain(0))
    g.quadrature_degree_used = h.quadrature_degree_used
    for c in (0, 7, msh.num_cells - 1):
        g._coeff = plain(c)
        want, _ = g._element_means(np.array([c]))
        assert np.allclose(got[c], want[0], rtol=1e-14, atol=0), c
    yq, w = h._quadrature_points()
    rows = np.concatenate([msh.cell_midpoints(), v], axis=1)
    assert np.allclose(got, h._coeff.host_stream(rows, yq, w), rtol=1e-14, atol=0)
    # one field as a 1-D array, and a callable evaluated at the midpoints
    one, _ = _solver(E("1.5 + f[0]*y[0]", fields=1))
    one.set_fields(v[:, 0])
    assert one._fields.shape == (msh.num_cells, 1) and np.array_equal(one._fields[:, 0], v[:, 0])
    one.set_fields(lambda x: 0.25 + x[0] * x[1])
    mid = msh.cell_midpoints()
    assert np.array_equal(one._fields[:, 0], 0.25 + mid[:, 0] * mid[:, 1])
    h.set_fields(lambda x: np.stack([0.25 + x[0], 0.5 - 0.25 * x[1]]))
    assert np.array_equal(h._fields, np.stack([0.25 + mid[:, 0], 0.5 - 0.25 * mid[:, 1]], axis=1))
    with pytest.raises(ValueError, match="need values of shape"):
        h.set_fields(lambda x: 0.25 + x[0])


def test_cell_means():
    h, msh = _solver()
    X = h.function_space.tabulate_dof_coordinates()
    u = 2.0 * X[:, 0] - 3.0 * X[:, 1] + 0.5  # affine: the mean of the vertex values is the value at the midpoint
    mid = msh.cell_midpoints()
    assert np.allclose(h.cell_means(u), 2.0 * mid[:, 0] - 3.0 * mid[:, 1] + 0.5, rtol=0, atol=1e-14)
    assert h.cell_means(u).shape == (msh.num_cells,)
    q = np.sin(X[:, 0]) + X[:, 1] ** 2
    assert np.allclose(h.cell_means(q), q[msh.cells].mean(axis=1), rtol=0, atol=1e-15)
    with pytest.raises(RuntimeError, match="cell_means"):
        h.cell_means()
    with pytest.raises(ValueError, match="dofs"):
        h.cell_means(u[:-1])
    h.set_fields(_values(msh))
    h.solve()
    assert np.array_equal(h.cell_means(), h.cell_means(h._u))
    e = hmm.LinearElasticityHMM(msh, hmm.Lame(1.0, 2.0) if False else (lambda x, y: hmm.Lame(1.0 + 0 * y[0], 2.0 + 0 * y[0])), lambda x: np.zeros(2),
                                mesh.create_unit_square(4, 4), 0.01)
    Xe = e.function_space.tabulate_dof_coordinates()
    ue = np.stack([Xe[:, 0] + 1.0, 2.0 * Xe[:, 1]], axis=1).ravel()  # dof = vertex * 2 + component
    got = e.cell_means(ue)
    assert got.shape == (msh.num_cells, 2) and np.allclose(got, np.stack([mid[:, 0] + 1.0, 2.0 * mid[:, 1]], axis=1), rtol=0, atol=1e-14)
