"""The stream-order contract of hommx_secant_load_source_device and hommx_secant_tangent_load_source_device on an MI355X (-m gpu;
DESIGN 4.18) under the in-flight protocol of tests/stream_order_gpu.py, on a fused plan (load solves by substitution on the factor
records), a blocked plan and a frontal mesh plan created with ``load_solve=True`` (substitution on its pivot columns).  The entries
queue ``max_iter`` rounds per chunk -- the eigenstress of the round, an elimination, a load solve and one launch of k_secant_load each
-- and for the tangent one launch of k_secant_tangent_load and one elimination on the sibling plan, and read nothing back: on a
non-blocking stream behind inputs that are still in flight, the eigenstrain among them, they must give, bit for bit, what the same
call gives on the null stream with everything synchronised.  The file sorts behind test_gpu_stream_order.py (the shared
plans of stream_order_gpu.py keep their scratch grown from one file to the next) and creates no stream outside the protocol.

The law is that of test_gpu_stream_order_secant.py; the load is a per-cell eigenstrain of order 0.3, so every input the entries read
(coef, M, xi, rows, E) reaches every floating-point output.
"""

import functools

import numpy as np
import pytest

import stream_order_gpu as H
from test_gpu_stream_order import CELLS, DELAY_MS
from test_gpu_stream_order_secant import ROUNDS, _law
from test_gpu_stream_order_secant import _inputs as _secant_inputs

pytestmark = pytest.mark.gpu

PLANS = {"fused2d_32": "fused2d_subst", "small_wave": "blocked", "mesh_front": "mesh_front_subst"}  # name -> route of the load solve
_cache = {}


@functools.lru_cache(maxsize=None)
def _plan(name):
    """The shared plan of stream_order_gpu.py; of the frontal mesh a plan of this file's own on the same mesh, with the load solve."""
    from hommx_amd import MicroCellPlan

    if name != "mesh_front":
        return H.plan(name)
    dim, _, kind, route, *_ = H.PLANS[name]
    return MicroCellPlan.from_mesh(H.mesh(dim), kind, route=route, load_solve=True)


@functools.lru_cache(maxsize=None)
def _sibling(name):
    from hommx_amd import MicroCellPlan

    dim, n, _, route, *_ = H.PLANS[name]
    kind = _plan(name).tangent_kind
    return MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(H.mesh(dim), kind, route=route)


def _inputs(name, nc, seed):
    d = dict(_secant_inputs(name, nc, seed))
    p = _plan(name)
    d["E"] = 0.3 * np.random.default_rng(277 + seed).integers(-8, 9, (nc, p.n_el, p.t)) / 8.0
    return d


def _outputs(p, nc):
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    return dict(H._tensor_outputs(p, nc), state=((nc, 3), H.F64), mean_flux=((nc, p.t), H.F64), coef_out=((nc,) + el, H.F64))


NAMES = ("coef", "M", "xi", "rows", "E")


def call_secant_load(name, p, nc, real, decoy):
    law = _law(p)
    return H.Call("secant_load", p, real, decoy, NAMES, _outputs(p, nc),
                  lambda a, st: p.secant_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, a["rows"], a["state"], a["A_eff"],
                                                max_iter=ROUNDS, tol=0.0, mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"],
                                                info_ptr=a["info"], stream=st, P_ptr=a["E"], eigenstrain=True))


def call_secant_tangent_load(name, p, nc, real, decoy):
    out = dict(_outputs(p, nc), tangent=((nc, p.t, p.t), H.F64), asymmetry=((nc,), H.F64),
               tangent_coef=((nc, p.n_el, p.t * (p.t + 1) // 2), H.F64))
    law, sib = _law(p), _sibling(name)
    return H.Call("secant_tangent_load", p, real, decoy, NAMES, out,
                  lambda a, st: p.secant_tangent_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, sib, a["rows"], a["state"],
                                                        a["A_eff"], a["tangent"], a["asymmetry"], max_iter=ROUNDS, tol=0.0,
                                                        mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"], info_ptr=a["info"],
                                                        tangent_coef_ptr=a["tangent_coef"], stream=st, P_ptr=a["E"], eigenstrain=True))


CALLS = {"secant": call_secant_load, "tangent": call_secant_tangent_load}


def _case(which, name):
    if (which, name) not in _cache:
        nc = CELLS[name]
        call = CALLS[which](name, _plan(name), nc, _inputs(name, nc, 1), _inputs(name, nc, 2))
        _cache[which, name] = (call,) + H.references(call)
    return _cache[which, name]


@pytest.mark.parametrize("name", list(PLANS))
@pytest.mark.parametrize("which", list(CALLS))
def test_load_device_entries_in_flight(which, name):
    assert _plan(name).load_kernel == PLANS[name]
    call, real, _ = _case(which, name)
    assert np.array_equal(real["state"][:, 0], np.full(CELLS[name], ROUNDS)) and np.array_equal(real["state"][:, 2], np.ones(CELLS[name]))
    H.in_flight(call, real, DELAY_MS)


def test_null_stream_calls_equal_the_host_entries():
    name = "fused2d_32"
    p, d = _plan(name), _inputs(name, CELLS[name], 1)
    kw = dict(rows=d["rows"], max_iter=ROUNDS, tol=0.0, return_coef=True, P=d["E"], eigenstrain=True)
    _, real, _ = _case("secant", name)
    r = p.secant(d["coef"], d["xi"], _law(p), d["M"], **kw)
    assert np.array_equal(real["state"], np.stack([r.rounds, r.change, r.status], axis=1).astype(np.float64))
    for k, a in (("A_eff", r.A_eff), ("mean_flux", r.mean_flux), ("coef_out", r.coef), ("info", r.info)):
        assert np.array_equal(real[k], a), k
    plain = p.secant(d["coef"], d["xi"], _law(p), d["M"], rows=d["rows"], max_iter=ROUNDS, tol=0.0)
    assert not np.array_equal(plain.mean_flux, r.mean_flux)  # the load reaches the outputs
    _, real, _ = _case("tangent", name)
    r = p.secant_tangent(d["coef"], d["xi"], _law(p), _sibling(name), d["M"], return_tangent_coef=True, **kw)
    for k, a in (("A_eff", r.A_eff), ("mean_flux", r.mean_flux), ("coef_out", r.coef), ("info", r.info), ("tangent", r.tangent),
                 ("asymmetry", r.asymmetry), ("tangent_coef", r.tangent_coef)):
        assert np.array_equal(real[k], a), k
