"""The grammar of a criterion that reads the nonlinear state (hommx_amd.expr.Criterion with ``b[k]`` and ``h[k]``): the two
names and their bounds, the row indices of ``program(t, n_comp)`` on every kind, the unchanged program of a criterion without them, and
``host_values`` against the formula written in NumPy.  No GPU, no library."""

import numpy as np
import pytest

from hommx_amd.expr import MAX_HISTORY, OP_STORE, OP_X, Criterion, SecantLaw

# kind -> (t, n_comp) in 2D and 3D
SIZES = {"poisson": {2: (2, 1), 3: (3, 1)}, "poisson_matrix": {2: (2, 3), 3: (3, 6)}, "elasticity": {2: (3, 2), 3: (6, 2)},
         "elasticity_voigt": {2: (3, 6), 3: (6, 21)}}
KINDS = [(k, d) for k in SIZES for d in (2, 3)]


# -- the two names ----------------------------------------------------------------------------------------------------------------------------
def test_b_and_h_are_state_names_of_a_criterion():
    c = Criterion("s[0]/where(b[1] > 20, 900, 60) + max(h[0], e[0])", history=2)
    assert c.state_indices == {"e": 1, "s": 1, "c": 0, "b": 2, "h": 1}
    assert c.reads_state and c.n_history == 2
    plain = Criterion("s[0]/where(c[1] > 20, 900, 60)")
    assert plain.state_indices == {"e": 0, "s": 1, "c": 2, "b": 0, "h": 0}
    assert not plain.reads_state and plain.n_history == 0
    assert Criterion("b[0]").reads_state and Criterion("h[1]", history=2).reads_state
    assert not Criterion("s[0]", history=2).reads_state and Criterion("s[0]", history=2).n_history == 2


def test_h_needs_the_keyword_and_its_index_the_declared_number():
    with pytest.raises(ValueError, match=r"h\[k\] needs"):
        Criterion("s[0] + h[0]")
    with pytest.raises(ValueError, match=r"below the number of history variables \(2\): Subscript 'h\[2\]'"):
        Criterion("h[2]", history=2)
    with pytest.raises(ValueError, match=r"Subscript 'h\[e\[0\]\]'"):
        Criterion("h[e[0]]", history=1)
    for bad in (0, MAX_HISTORY + 1, -1, 1.0, True, "1", [1]):
        with pytest.raises(ValueError, match=rf"history is the number of history variables, 1 .. {MAX_HISTORY}"):
            Criterion("s[0]", history=bad)
    assert Criterion("h[3]", history=MAX_HISTORY).state_indices["h"] == 4


def test_the_index_of_b_is_a_literal_checked_against_the_plan():
    with pytest.raises(ValueError, match=r"the index of b is a literal integer 0 .. 20"):
        Criterion("b[21]")
    with pytest.raises(ValueError, match=r"the index of b is a literal integer"):
        Criterion("b[-1]")
    c = Criterion("b[2]")
    with pytest.raises(ValueError, match=r"criterion: b\[2\] is out of range: the plan has n_comp = 2 \(t = 3, n_comp = 2\)"):
        c.program(3, 2)
    assert c.program(3, 6)[0].tolist() == [[OP_X, 3 + 6 + 6 + 2], [OP_STORE, 0]]
    with pytest.raises(ValueError, match="unknown name|only x and y are indexed"):
        SecantLaw("b[0]")  # a law has no b: its c is the base


def test_a_strength_text_of_the_builders_may_read_b():
    c = Criterion.von_mises(2, strength="where(b[1] > 20, 900, 60)")
    assert c.reads_state and c.state_indices["b"] == 2 and c.state_indices["c"] == 1
    assert Criterion.max_principal(strength="b[0]").reads_state and not Criterion.max_principal().reads_state
    assert not Criterion.flux_norm("elasticity", 2).reads_state


# -- the row ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", KINDS)
@pytest.mark.parametrize("n_fields,n_history", [(0, 0), (0, 1), (2, 4), (1, 0)])
def test_row_indices_of_every_name_on_every_kind(kind, dim, n_fields, n_history):
    t, n_comp = SIZES[kind][dim]
    kw = dict(fields=n_fields or None, history=n_history or None)
    base = 3 + n_fields
    k = n_comp - 1
    want = {f"e[{t - 1}]": base + t - 1, f"s[{t - 1}]": base + 2 * t - 1, f"c[{k}]": base + 2 * t + k,
            f"b[{k}]": base + 2 * t + n_comp + n_history + k, "b[0]": base + 2 * t + n_comp + n_history}
    if n_history:
        want[f"h[{n_history - 1}]"] = base + 2 * t + n_comp + n_history - 1
        want["h[0]"] = base + 2 * t + n_comp  # the index it has in a SecantLaw
    for text, index in want.items():
        ops, consts = Criterion(text, **kw).program(t, n_comp)
        assert ops.tolist() == [[OP_X, index], [OP_STORE, 0]] and consts.size == 0, text
    if n_history:
        law = SecantLaw(["c[0]"] * n_comp if n_comp > 1 else "c[0]", history=["h[0]"] * n_history, fields=n_fields or None) \
            if kind != "poisson_matrix" and kind != "elasticity" else None
        if law is not None:
            ops, _ = law.program(t, n_comp)
            assert ops[-2].tolist() == [OP_X, want["h[0]"]]


def test_an_undeclared_criterion_stands_on_the_row_of_any_law_and_a_declared_one_on_its_own():
    c = Criterion("b[1]")
    assert c.program(3, 2)[0][0].tolist() == [OP_X, 3 + 6 + 2 + 1]
    assert c.program(3, 2, 3)[0][0].tolist() == [OP_X, 3 + 6 + 2 + 3 + 1]  # behind the three history entries of the law
    d = Criterion("b[1] + h[0]", history=2)
    assert d.program(3, 2, 2)[0][:2].tolist() == [[OP_X, 3 + 6 + 2 + 2 + 1], [OP_X, 3 + 6 + 2]]
    with pytest.raises(ValueError, match=r"declares history=2; the law has 3 history variables"):
        d.program(3, 2, 3)
    with pytest.raises(ValueError, match=r"declares history=2; the law has 0 history variables"):
        d.program(3, 2, 0)


@pytest.mark.parametrize("kind,dim", KINDS)
def test_a_criterion_without_the_names_has_the_program_it_had(kind, dim):
    """The expected arrays are written out from the row of section 4.14, [midpoint 3 | fields | e | s | c]: nothing of them depends on
    the two new names, and ``history=`` alone changes nothing either."""
    t, n_comp = SIZES[kind][dim]
    text = f"where(c[{n_comp - 1}] > 2, s[{t - 1}], e[0])*f[1] + p[0]"
    for kw in ({}, {"history": 3}):
        ops, consts = Criterion(text, p=[0.5], fields=2, **kw).program(t, n_comp)
        x = [c for o, c in ops.tolist() if o == OP_X]
        assert x == [5 + 2 * t + n_comp - 1, 5 + 2 * t - 1, 5, 4]
        assert np.array_equal(consts, [0.5, 2.0]) and ops[-1].tolist() == [OP_STORE, 0]
        assert np.array_equal(ops, Criterion(text, p=[0.5], fields=2).program(t, n_comp)[0])
    vm = Criterion.von_mises(dim)
    assert np.array_equal(vm.program(6 if dim == 3 else 3, 2)[0], Criterion(vm.text).program(6 if dim == 3 else 3, 2)[0])


# -- host_values ------------------------------------------------------------------------------------------------------------------------------
def _state(rng, N=3, n_el=7, t=3, n_comp=2, nh=2):
    return dict(e=rng.standard_normal((N, n_el, t)), s=rng.standard_normal((N, n_el, t)), c=rng.uniform(1, 2, (N, n_el, n_comp)),
                b=rng.uniform(2, 3, (N, n_el, n_comp)), h=rng.uniform(0, 1, (N, n_el, nh)), x=rng.standard_normal((N, 3)),
                y=rng.uniform(0, 1, (n_el, 2)), f=rng.standard_normal((N, 1)))


def test_host_values_against_the_formula():
    d = _state(np.random.default_rng(5))
    crit = Criterion("max(h[1], sqrt(e[0]**2 + e[1]**2))*b[1]/c[1] + where(b[0] > 2.5, s[2], f[0])*y[1] - h[0]*x[0]", fields=1, history=2)
    got = crit.host_values(d["e"], d["s"], d["c"], d["x"], d["y"], d["f"], base=d["b"], history=d["h"])
    e, s, c, b, h = d["e"], d["s"], d["c"], d["b"], d["h"]
    want = np.maximum(h[..., 1], np.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2)) * b[..., 1] / c[..., 1] \
        + np.where(b[..., 0] > 2.5, s[..., 2], d["f"][:, :1]) * d["y"][None, :, 1] - h[..., 0] * d["x"][:, :1]
    assert got.shape == (3, 7) and np.array_equal(got, want)
    # scalar coefficient and one history variable without their last axis
    d1 = _state(np.random.default_rng(6), t=2, n_comp=1, nh=1)
    one = Criterion("b[0]*h[0] - c[0]*s[1]", history=1)
    got = one.host_values(d1["e"], d1["s"], d1["c"][..., 0], d1["x"], base=d1["b"][..., 0], history=d1["h"][..., 0])
    assert np.array_equal(got, d1["b"][..., 0] * d1["h"][..., 0] - d1["c"][..., 0] * d1["s"][..., 1])


def test_host_values_of_an_undeclared_criterion_on_the_row_of_a_law_with_history():
    d = _state(np.random.default_rng(7))
    crit = Criterion("b[1] - c[1]")
    want = d["b"][..., 1] - d["c"][..., 1]
    assert np.array_equal(crit.host_values(d["e"], d["s"], d["c"], d["x"], base=d["b"]), want)
    assert np.array_equal(crit.host_values(d["e"], d["s"], d["c"], d["x"], base=d["b"], history=d["h"]), want)


def test_host_values_names_the_array_that_is_missing():
    d = _state(np.random.default_rng(8))
    args = (d["e"], d["s"], d["c"], d["x"])
    with pytest.raises(ValueError, match=r"the criterion reads b\[1\]: pass the base coefficient stream base\[N, n_el, 2\]"):
        Criterion("b[1]").host_values(*args)
    with pytest.raises(ValueError, match=r"the criterion reads h\[0\]: pass history\[N, n_el, 2\]"):
        Criterion("h[0]", history=2).host_values(*args, base=d["b"])
    with pytest.raises(ValueError, match=r"base must have the shape of c"):
        Criterion("b[1]").host_values(*args, base=d["b"][:, :, :1])
    with pytest.raises(ValueError, match=r"history must be \[N, n_el, n_history\]"):
        Criterion("h[0]", history=2).host_values(*args, history=d["h"][:, :3])
    with pytest.raises(ValueError, match=r"declares history=2; the law has 1"):
        Criterion("h[0]", history=2).host_values(*args, history=d["h"][:, :, :1])
    # a criterion that reads neither takes neither, and the linear call is the one it was
    plain = Criterion("s[0]*c[1]")
    assert np.array_equal(plain.host_values(*args), d["s"][..., 0] * d["c"][..., 1])
    assert np.array_equal(plain.host_values(*args, base=d["b"], history=d["h"]), d["s"][..., 0] * d["c"][..., 1])
