"""The stream-order contract of hommx_secant_tangent_source_device on an MI355X (-m gpu) under the in-flight protocol of
tests/stream_order_gpu.py, on the five plans of test_gpu_stream_order_secant.py.  The entry queues, per chunk, ``max_iter`` rounds, one
launch of k_secant_tangent and one elimination on the SIBLING plan, whose own scratch is touched on the caller's stream as well, and
reads nothing back: on a non-blocking stream behind inputs that are still in flight it must give, bit for bit, what the same call
gives on the null stream with everything synchronised.  The file sorts behind test_gpu_stream_order_secant.py (the shared
plans of stream_order_gpu.py keep their scratch grown from one file to the next).

The law is that file's: every input the entry reads (coef, M, xi, rows) reaches every floating-point output, the tangent included.
"""

import functools

import numpy as np
import pytest

import stream_order_gpu as H
from test_gpu_stream_order import CELLS, DELAY_MS
from test_gpu_stream_order_secant import PLANS, ROUNDS, _inputs, _law

pytestmark = pytest.mark.gpu

_cache = {}


@functools.lru_cache(maxsize=None)
def _sibling(name):
    from hommx_amd import MicroCellPlan

    dim, n, _, route, *_ = H.PLANS[name]
    kind = H.plan(name).tangent_kind
    return MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(H.mesh(dim), kind, route=route)


def call_secant_tangent(name, p, nc, real, decoy):
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    out = dict(H._tensor_outputs(p, nc), state=((nc, 3), H.F64), mean_flux=((nc, p.t), H.F64), coef_out=((nc,) + el, H.F64),
               tangent=((nc, p.t, p.t), H.F64), asymmetry=((nc,), H.F64), tangent_coef=((nc, p.n_el, p.t * (p.t + 1) // 2), H.F64))
    # tangent_info is not asked for: it is zero for real and decoy inputs alike, and the protocol wants outputs that tell them apart
    law, sib = _law(p), _sibling(name)
    return H.Call("secant_tangent", p, real, decoy, ("coef", "M", "xi", "rows"), out,
                  lambda a, st: p.secant_tangent_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, sib, a["rows"], a["state"],
                                                        a["A_eff"], a["tangent"], a["asymmetry"], max_iter=ROUNDS, tol=0.0,
                                                        mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"], info_ptr=a["info"],
                                                        tangent_coef_ptr=a["tangent_coef"], stream=st))


def _case(name):
    if name not in _cache:
        nc = CELLS[name]
        call = call_secant_tangent(name, H.plan(name), nc, _inputs(name, nc, 1), _inputs(name, nc, 2))
        _cache[name] = (call,) + H.references(call)
    return _cache[name]


@pytest.mark.parametrize("name", PLANS)
def test_secant_tangent_device_in_flight(name):
    call, real, _ = _case(name)
    assert np.array_equal(real["state"][:, 2], np.ones(CELLS[name])) and not np.array_equal(real["tangent"], real["A_eff"])
    H.in_flight(call, real, DELAY_MS)


def test_null_stream_call_equals_the_host_entry():
    name = "small_wave"
    call, real, _ = _case(name)
    p, d = H.plan(name), _inputs(name, CELLS[name], 1)
    r = p.secant_tangent(d["coef"], d["xi"], _law(p), _sibling(name), d["M"], rows=d["rows"], max_iter=ROUNDS, tol=0.0, return_coef=True,
                         return_tangent_coef=True)
    assert np.array_equal(real["state"], np.stack([r.rounds, r.change, r.status], axis=1).astype(np.float64))
    for k, a in (("A_eff", r.A_eff), ("mean_flux", r.mean_flux), ("coef_out", r.coef), ("info", r.info), ("tangent", r.tangent),
                 ("asymmetry", r.asymmetry), ("tangent_coef", r.tangent_coef)):
        assert np.array_equal(real[k], a), k
