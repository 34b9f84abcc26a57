"""The stream-order contract of hommx_secant_source_device on an MI355X (-m gpu): "asynchronous on `stream`" (include/hommx_hip.h,
hommx_solve_batch_device) under the in-flight protocol of tests/stream_order_gpu.py.  The entry queues exactly ``max_iter`` rounds per
chunk -- an elimination and one launch of k_secant_update each, between a device-to-device copy of the start stream and one of the
result -- and reads nothing back, so it never waits for its own work: on a non-blocking stream behind inputs that are still in flight
it must give, bit for bit, what the same call gives on the null stream with everything synchronised.  One self-check shows that the
protocol notices a call that does not wait for its inputs.

The law scales every entry of the base coefficient by 0.5 + 0.5 / (1 + e0^2 + e1^2) and adds the first midpoint coordinate to entry 0
times 2^-6, so every input the entry reads (coef, M, xi, rows) reaches every floating-point output.  Eight rounds at tol = 0: every cell
runs to ``max_iter`` (status 1), whatever its inputs, so real and decoy outputs differ everywhere.  The delay is that of
test_gpu_stream_order.py: eight rounds of its "reconstruct" column stay below 8 x 0.71 ms.
"""

import numpy as np
import pytest

import stream_order_gpu as H
from test_gpu_stream_order import CELLS, DELAY_MS

pytestmark = pytest.mark.gpu

PLANS = ["fused2d_32", "small_wave", "multifrontal", "mesh_front", "mesh_tree"]
ROUNDS = 8
_cache = {}


def _law(p):
    from hommx_amd.expr import SecantLaw

    soft = "(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))"
    texts = [f"c[{k}]*{soft}" + (" + 0.015625*abs(x[0])*c[0]" if k == 0 else "") for k in range(p.n_comp)]
    return SecantLaw(texts[0]) if p.n_comp == 1 else SecantLaw(lam=texts[0], mu=texts[1])


def _inputs(name, nc, seed):
    d = dict(H.inputs(name, nc, seed))
    d["rows"] = np.random.default_rng(77 + seed).integers(1, 9, (nc, 3)) / 8.0
    return d


def call_secant(p, nc, real, decoy):
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    out = dict(H._tensor_outputs(p, nc), state=((nc, 3), H.F64), mean_flux=((nc, p.t), H.F64), coef_out=((nc,) + el, H.F64))
    law = _law(p)
    return H.Call("secant", p, real, decoy, ("coef", "M", "xi", "rows"), out,
                  lambda a, st: p.secant_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, a["rows"], a["state"], a["A_eff"],
                                                max_iter=ROUNDS, tol=0.0, mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"],
                                                info_ptr=a["info"], stream=st))


def _case(name):
    if name not in _cache:
        nc = CELLS[name]
        call = call_secant(H.plan(name), nc, _inputs(name, nc, 1), _inputs(name, nc, 2))
        _cache[name] = (call,) + H.references(call)
    return _cache[name]


@pytest.mark.parametrize("name", PLANS)
def test_secant_device_in_flight(name):
    call, real, _ = _case(name)
    assert np.array_equal(real["state"][:, 0], np.full(CELLS[name], ROUNDS)) and np.array_equal(real["state"][:, 2], np.ones(CELLS[name]))
    H.in_flight(call, real, DELAY_MS)


def test_null_stream_call_equals_the_host_entry():
    """The bits of the null-stream reference are those of the host entry, which stops reading the state after every round."""
    name = "fused2d_32"
    call, real, _ = _case(name)
    p, nc, d = H.plan(name), CELLS[name], _inputs(name, CELLS[name], 1)
    r = p.secant(d["coef"], d["xi"], _law(p), d["M"], rows=d["rows"], max_iter=ROUNDS, tol=0.0, return_coef=True)
    assert np.array_equal(real["state"], np.stack([r.rounds, r.change, r.status], axis=1).astype(np.float64))
    for k, a in (("A_eff", r.A_eff), ("mean_flux", r.mean_flux), ("coef_out", r.coef), ("info", r.info)):
        assert np.array_equal(real[k], a), k


def test_protocol_sees_a_call_that_does_not_wait():
    call, real, decoy = _case("fused2d_32")
    H.unordered(call, real, decoy, DELAY_MS)
