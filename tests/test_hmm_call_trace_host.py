"""What the solver classes send to their plan, and what they return, against the trace recorded from the commit before the Python
layer was folded onto one chunk driver (tests/golden/hmm_calls/, written by tools/record_hmm_calls.py -- the cases are listed there).

Every case is run again on a recording stand-in plan and must give the same sequence of calls with the same keywords, the same
streams, shapes, dtypes and chunk boundaries, the same result fields, ``quadrature_degree_used``, WARNING lines and, for a refusal, the
same exception type and text after the same calls.  Strings, integer, bool and uint8 arrays are equal exactly; float arrays to within
``BOUND`` of the array's largest magnitude -- they are not bitwise across machines: ``tensordot``, ``einsum``, the (d + 1) x (d + 1)
inverse of ``_strain_basis`` and the sparse macro solve go through whatever BLAS / LAPACK / SuperLU the machine has.  No GPU needed."""

import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "hmm_calls")

# Largest deviation of any float array, in units of its largest magnitude.  Measured by replaying the fixture against the commit it was
# recorded from: 0 on the machine that recorded it (the recorder is deterministic) and MEASURED on a second machine (the one with
# the MI355X, its own Python, NumPy and SciPy): 0.0 there as well, in all 964 cases.  Allowed: twice that, and at least 4 ulp -- the
# inputs are sums of at most six products and one small inverse on a uniform mesh.
MEASURED = 0.0
BOUND = max(2.0 * MEASURED, 4.0 * np.finfo(np.float64).eps)


def _recorder():
    spec = importlib.util.spec_from_file_location("record_hmm_calls", os.path.join(os.path.dirname(HERE), "tools", "record_hmm_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def traces():
    """(recorded index, recorded arrays, index of this tree, arrays of this tree): recorded once for all the tests."""
    recorder = _recorder()
    want, want_arrays = recorder.load(GOLDEN)
    got, got_arrays = recorder.record()
    return want, want_arrays, json.loads(json.dumps(got)), got_arrays


def deviation(want: np.ndarray, got: np.ndarray, where: str) -> float:
    """Shape and dtype equal; exact arrays equal; the deviation of a float array in units of its largest magnitude."""
    assert want.shape == got.shape and want.dtype == got.dtype, f"{where}: {got.dtype}{got.shape}, recorded {want.dtype}{want.shape}"
    if want.dtype.kind != "f":
        assert np.array_equal(want, got), where
        return 0.0
    assert np.array_equal(np.isnan(want), np.isnan(got)), where
    scale = float(np.nanmax(np.abs(want), initial=0.0))
    dev = float(np.nanmax(np.abs(want - got), initial=0.0))
    return dev / scale if scale > 0 else dev


def compare(want, got, want_arrays, got_arrays, where: str) -> float:
    """Walk two recorded values together; returns the largest deviation of the float arrays below them."""
    if isinstance(want, dict) and set(want) == {"array"}:
        assert isinstance(got, dict) and set(got) == {"array"}, where
        return deviation(want_arrays[want["array"]], got_arrays[got["array"]], where)
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(want) == sorted(got), f"{where}: {sorted(got) if isinstance(got, dict) else got}, recorded {sorted(want)}"
        return max((compare(want[k], got[k], want_arrays, got_arrays, f"{where}.{k}") for k in want), default=0.0)
    if isinstance(want, list):
        assert isinstance(got, list) and len(want) == len(got), f"{where}: {len(got) if isinstance(got, list) else got} entries, recorded {len(want)}"
        return max((compare(w, g, want_arrays, got_arrays, f"{where}[{k}]") for k, (w, g) in enumerate(zip(want, got))), default=0.0)
    assert type(want) is type(got) and want == got, f"{where}: {got!r}, recorded {want!r}"
    return 0.0


def test_the_cases_are_the_recorded_ones(traces):
    want, _, got, _ = traces
    assert sorted(want) == sorted(got)
    assert len(want) > 900 and sum("raises" in c for c in want.values()) > 300
    chunked = [k for k in want if k.endswith("/chunk5") and "raises" not in want[k]]
    assert chunked and all(len(want[k]["calls"]) >= 2 for k in chunked)  # 7 cells: 2 chunks, 32: 7, 48: 10
    with open(os.path.join(GOLDEN, "index.json")) as f:  # the readable index says what the trace holds
        assert json.load(f) == {k: {"calls": [c["method"] for c in v["calls"]], "raises": v.get("raises", [None])[0]} for k, v in want.items()}


@pytest.mark.parametrize("tag", ["means", "sampler"])
@pytest.mark.parametrize("solver", ["callable", "two_phase", "affine", "reciprocal", "expression", "expression_curved", "lame", "stratified",
                                    "lame3d", "periodic"])
def test_calls_and_results_are_the_recorded_ones(traces, tag, solver):
    want, want_arrays, got, got_arrays = traces
    names = [k for k in want if k.startswith(f"{tag}/{solver}/")]
    assert names
    worst, at = 0.0, None
    for name in names:
        w, g = want[name], got[name]
        assert [c["method"] for c in g["calls"]] == [c["method"] for c in w["calls"]], name
        assert g.get("raises") == w.get("raises"), name
        dev = compare(w, g, want_arrays, got_arrays, name)
        if dev > worst:
            worst, at = dev, name
    print(f"{tag}/{solver}: {len(names)} cases, largest deviation {worst:.3e} of the largest magnitude" + (f" ({at})" if at else ""))
    assert worst <= BOUND, f"{at}: {worst:.3e} > {BOUND:.3e}"
