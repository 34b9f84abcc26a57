"""The stream-order contract of hommx_loads_source_device and hommx_second_sensitivity_source_device on plans whose load solve
substitutes on the kept fronts (HOMMX_FLAG_TREE_LOADS / HOMMX_MESH_FLAG_TREE_LOADS) on an MI355X (-m gpu), under the
in-flight protocol of tests/stream_order_gpu.py: one flagged structured plan (3D elasticity 5^3) and one flagged mesh plan (3D Poisson on
the jittered cube, created with HOMMX_MF_LEAF = 8 so that its tree has several levels -- tests/test_gpu_tree_loads.py).  At 40 cells the
canonical pass runs as two pieces, one on a plan-owned side stream; the load solve takes over those pieces and that stream, forks behind
the caller's stream and joins it again: on a non-blocking stream behind inputs that are still in flight both entries must give, bit for
bit, what the same call gives on the null stream with everything synchronised.  The file sorts behind
test_gpu_stream_order_secant_load.py (DESIGN 4.15 on the stream count) and creates no stream outside the protocol."""

import functools

import numpy as np
import pytest

import stream_order_gpu as H
from test_gpu_stream_order import CELLS, DELAY_MS
from test_gpu_tree_loads import plan as flagged_plan

pytestmark = pytest.mark.gpu

PLANS = {"multifrontal": "multifrontal", "mesh_tree": "mesh_tree_3d"}  # input set of stream_order_gpu.PLANS -> case of test_gpu_tree_loads


@functools.lru_cache(maxsize=None)
def _plan(name):
    p = flagged_plan(PLANS[name])
    dim, n, kind, *_ = H.PLANS[name]
    assert (p.dim, p.n_micro, p.kind) == (dim, n, kind) and p.load_kernel.endswith("_subst")
    assert p.n_el == H.plan(name).n_el  # the input sets of stream_order_gpu fit this plan
    return p


def _calls(name):
    p, nc = _plan(name), CELLS[name]
    assert nc >= 16  # two pieces: the side stream is in play
    real, decoy = H.inputs(name, nc, 1), H.inputs(name, nc, 2)
    out = {"A_eff": ((nc, p.t, p.t), H.F64), "info": ((nc,), H.I32), "d2A": ((nc, 2, 2, p.t, p.t), H.F64), "dA": ((nc, 2, p.t, p.t), H.F64)}
    sens2 = H.Call("second_sensitivities", p, real, decoy, ("coef", "M", "dirs"), out,
                   lambda a, st: p.second_sensitivities_device(nc, H._source(a, "sampled"), a["M"], 2, a["dirs"], a["d2A"], False, a["dA"],
                                                               a["A_eff"], a["info"], st))
    return {"loads": H.call_loads(p, nc, real, decoy), "second_sensitivities": sens2}


@pytest.mark.parametrize("entry", ["loads", "second_sensitivities"])
@pytest.mark.parametrize("name", list(PLANS))
def test_device_entries_in_flight(name, entry):
    call = _calls(name)[entry]
    real, _ = H.references(call)
    H.in_flight(call, real, DELAY_MS)


@pytest.mark.parametrize("name", list(PLANS))
def test_null_stream_call_equals_the_host_entry(name):
    p, nc = _plan(name), CELLS[name]
    d = H.inputs(name, nc, 1)
    real = H.reference(_calls(name)["loads"], 0)
    r = p.loads(d["coef"], d["P"], d["M"], response=True, return_correctors=True)
    for k, a in (("A_eff", r.A_eff), ("P_eff", r.P_eff), ("energy", r.energy), ("correctors", r.correctors), ("info", r.info)):
        assert np.array_equal(real[k], a), k
