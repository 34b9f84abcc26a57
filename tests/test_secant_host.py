"""Strain-dependent coefficients on the CPU: the grammar and the component shapes of ``SecantLaw``, the component count against the plan's
``n_comp``, the ``X`` indices its program reads the state through, and ``host_values`` -- the NumPy twin the device is held to -- against
the formula written out in NumPy on dyadic data (no GPU needed)."""

import numpy as np
import pytest

from hommx_amd import hmm
from hommx_amd.expr import OP_STORE, OP_X, OP_Y, Expression, SecantLaw

SOFT = "c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"


def test_hmm_exports_the_law():
    assert hmm.SecantLaw is SecantLaw


def test_component_shapes():
    assert (SecantLaw(SOFT).shape, SecantLaw(SOFT).n_comp) == ("scalar", 1)
    lame = SecantLaw(lam="c[0]", mu="c[1]/(1 + e[2]**2)")
    assert (lame.shape, lame.n_comp) == ("lame", 2)
    m2 = SecantLaw([["c[0]", "c[2]*s[0]"], ["c[2]*s[0]", "c[1]"]])
    assert (m2.shape, m2.dim, m2.n_comp, m2.texts) == ("matrix", 2, 3, ("c[0]", "c[1]", "c[2]*s[0]"))  # the poisson_matrix order
    m3 = SecantLaw([[f"c[{max(i, j)}]" for j in range(3)] for i in range(3)])
    assert m3.n_comp == 6 and m3.texts == ("c[0]", "c[1]", "c[2]", "c[1]", "c[2]", "c[2]")  # (0,0) (1,1) (2,2) (0,1) (0,2) (1,2)
    voigt = SecantLaw([f"c[{k}]" for k in range(21)])
    assert (voigt.shape, voigt.n_comp) == ("vector", 21)


def test_parser_refusals():
    with pytest.raises(ValueError, match="SecantLaw\\(text\\)"):
        SecantLaw()
    with pytest.raises(ValueError, match="SecantLaw\\(text\\)"):
        SecantLaw("c[0]", lam="c[0]", mu="c[1]")
    with pytest.raises(ValueError, match="SecantLaw\\(text\\)"):
        SecantLaw(lam="c[0]")
    with pytest.raises(ValueError, match="symmetric"):
        SecantLaw([["c[0]", "c[1]"], ["c[2]", "c[0]"]])
    with pytest.raises(ValueError, match="2 x 2 or 3 x 3"):
        SecantLaw([["c[0]", "c[1]", "c[2]"], ["c[1]", "c[0]", "c[2]"]])
    with pytest.raises(ValueError, match="1 .. 21 components"):
        SecantLaw(["c[0]"] * 22)
    with pytest.raises(ValueError, match="too long"):
        SecantLaw([SOFT] * 9)  # 9 x 16 instructions
    with pytest.raises(ValueError):
        SecantLaw("q[0]")  # no such name
    with pytest.raises(ValueError):
        SecantLaw("c[21]")  # above the largest index a state name can have
    with pytest.raises(ValueError):
        SecantLaw("c[0]*f[0]")  # a field without fields=
    with pytest.raises(ValueError):
        SecantLaw("c[0]*p[1]", p=[1.0])
    with pytest.raises(ValueError, match="parameter_names"):
        SecantLaw("c[0]*p[0]", p=[1.0], parameter_names=("a", "b"))
    deep = "c[0]"
    for i in range(16):
        deep = f"(e[{i % 2}] - {deep})"
    with pytest.raises(ValueError, match="too deep"):
        SecantLaw(deep)
    for name in "esc":  # the state names are a law's (and a criterion's) alone
        with pytest.raises(ValueError):
            Expression(f"1 + {name}[0]")


def test_component_count_and_index_ranges_are_checked_when_the_law_meets_a_plan():
    with pytest.raises(ValueError, match="it has 1 components; the plan's coefficient has n_comp = 2"):
        SecantLaw(SOFT).program(3, 2)
    with pytest.raises(ValueError, match="it has 2 components; the plan's coefficient has n_comp = 1"):
        SecantLaw(lam="c[0]", mu="c[0]").program(2, 1)
    with pytest.raises(ValueError, match="e\\[2\\] is out of range: the plan has t = 2"):
        SecantLaw("c[0]/(1 + e[2]**2)").program(2, 1)
    with pytest.raises(ValueError, match="s\\[3\\] is out of range: the plan has t = 3"):
        SecantLaw(lam="c[0]", mu="c[1] + s[3]").program(3, 2)
    with pytest.raises(ValueError, match="c\\[1\\] is out of range: the plan has n_comp = 1"):
        SecantLaw("c[1]").program(2, 1)


def test_the_state_is_read_through_x_on_the_row_of_a_criterion():
    law = SecantLaw(lam="c[0] + f[1]*e[2]", mu="c[1]*s[0] + x[1] + y[0]", fields=2)
    ops, consts = law.program(3, 2)  # row: [midpoint 3 | fields 2 | e 3 | s 3 | c 2]
    assert [int(k) for op, k in ops if op == OP_X] == [11, 4, 7, 12, 8, 1]
    assert [int(k) for op, k in ops if op == OP_STORE] == [0, 1] and ops[-1].tolist() == [OP_STORE, 1]
    assert [int(k) for op, k in ops if op == OP_Y] == [0] and law.n_y == 1
    assert law.state_indices == {"e": 3, "s": 1, "c": 2}
    assert ops.dtype == np.uint8 and ops.shape[1] == 2 and ops[:, 0].max() <= OP_STORE  # no opcode is added
    ops6, _ = law.program(6, 2)
    assert [int(k) for op, k in ops6 if op == OP_X] == [17, 4, 7, 18, 11, 1]


def test_with_parameters_changes_the_constants_alone():
    law = SecantLaw("c[0]*(p[0] + p[1]/(1 + e[0]**2))", p=[0.5, 0.5], parameter_names=("floor", "drop"))
    other = law.with_parameters([0.25, 0.75])
    assert np.array_equal(law.p, [0.5, 0.5]) and np.array_equal(other.p, [0.25, 0.75])
    assert np.array_equal(law.program(2, 1)[0], other.program(2, 1)[0])
    with pytest.raises(ValueError):
        law.with_parameters([1.0])


def _dyadic(rng, *shape):
    return rng.integers(-16, 17, shape) / 8.0


def test_host_values_is_the_formula():
    rng = np.random.default_rng(3)
    N, n_el = 3, 7
    e, s = _dyadic(rng, N, n_el, 2), _dyadic(rng, N, n_el, 2)
    c = 1.0 + np.abs(_dyadic(rng, N, n_el))
    x, y, f = _dyadic(rng, N, 3), _dyadic(rng, n_el, 2), _dyadic(rng, N, 1)
    got = SecantLaw(SOFT).host_values(e, s, c, x)
    assert got.shape == (N, n_el, 1)
    assert np.array_equal(got[..., 0], c * (0.5 + 0.5 / (1 + e[..., 0] ** 2 + e[..., 1] ** 2)))
    law = SecantLaw("where(c[0] > 2, c[0], c[0]*p[0]) + f[0]*s[1] - x[2]*y[1]", p=[0.25], fields=1)
    want = np.where(c > 2, c, c * 0.25) + f[:, :1] * s[..., 1] - x[:, 2:3] * y[None, :, 1]
    assert np.array_equal(law.host_values(e, s, c, x, y, f)[..., 0], want)
    with pytest.raises(ValueError, match="fields"):
        law.host_values(e, s, c, x, y)
    with pytest.raises(ValueError, match="centroids"):
        law.host_values(e, s, c, x, None, f)
    # two components on t = 3: the order of the stores is the order of the last axis
    e3, s3, c2 = _dyadic(rng, N, n_el, 3), _dyadic(rng, N, n_el, 3), 1.0 + np.abs(_dyadic(rng, N, n_el, 2))
    lame = SecantLaw(lam="c[0]", mu="c[1]/(1 + (e[0] - e[1])**2 + e[2]**2)")
    got = lame.host_values(e3, s3, c2, x)
    assert got.shape == (N, n_el, 2) and np.array_equal(got[..., 0], c2[..., 0])
    assert np.array_equal(got[..., 1], c2[..., 1] / (1 + (e3[..., 0] - e3[..., 1]) ** 2 + e3[..., 2] ** 2))
    with pytest.raises(ValueError, match="n_comp = 1"):
        lame.host_values(e, s, c, x)
