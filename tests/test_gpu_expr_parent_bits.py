"""The one interpreter kernel k_expand_program<P> (csrc/coef_program.hip) against the two kernels it replaced, on an MI355X (-m gpu).

tests/golden/expr_streams/expr_streams_parent.npz holds, as raw float64, what ``MicroCellPlan.expand`` and ``expand_tangents`` gave for
the programs of tests/expr_stream_cases.py with the library built from the commit BEFORE the value kernel and the forward-mode
kernel became one template (tools/record_expr_streams.py wrote it there; never the code under test).  The library must reproduce
every array bit for bit: the value pass (P = 0) of every program, and the value stream and the tangents of the forward-mode pass (P = 1, 2, 4) of every program
with slots.  The cases and what they cover: the docstring of expr_stream_cases.py.

The bits of sqrt, sin, cos, tan, exp, log and tanh are those of the device math library of the toolchain, whose version the fixture
records (``rocm``): with a toolchain whose device math library differs, the fixture has to be recorded again from the commit before
this test was added, not from the tree under test.
"""

import functools
import os

import numpy as np
import pytest

import expr_stream_cases as S

pytestmark = pytest.mark.gpu

CASES = S.cases()


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expr_streams", "expr_streams_parent.npz"))


@functools.lru_cache(maxsize=None)
def _plan(shape):
    return S.plan(shape)


def test_the_fixture_holds_every_case_and_names_its_toolchain():
    g = _golden()
    want = {f"{name}/{key}" for name, _, A in CASES for key in ("ops", "consts", "coef") + (("dirs",) if A.n_params + A.n_fields else ())}
    assert set(g.files) == want | {"rocm"}
    print("recorded with ROCm", g["rocm"])
    assert str(g["rocm"])


@pytest.mark.parametrize("name,shape,A", CASES, ids=[c[0] for c in CASES])
def test_streams_and_tangents_are_the_parent_commits_bitwise(name, shape, A):
    g = _golden()
    ops, consts = A.program()
    assert np.array_equal(ops, g[f"{name}/ops"]) and np.array_equal(consts, g[f"{name}/consts"])  # the program the numbers belong to
    p, stream = _plan(shape), S.stream(shape, A)
    n_tan = A.n_params + A.n_fields
    assert g[f"{name}/coef"].shape[:2] == (len(stream), p.n_el) and (len(stream) * p.n_el) % 64 != 0
    assert np.array_equal(p.expand(stream), g[f"{name}/coef"])
    if n_tan:
        coef, dirs = p.expand_tangents(stream)
        assert dirs.shape[:3] == (len(stream), n_tan, p.n_el)
        assert np.array_equal(coef, g[f"{name}/coef"])
        assert np.array_equal(dirs, g[f"{name}/dirs"])
