"""The stream-order contract of hommx_secant_history_source_device and hommx_secant_tangent_history_source_device on an MI355X
(-m gpu) under the in-flight protocol of tests/stream_order_gpu.py, on the five plans of test_gpu_stream_order_secant.py.
The entries queue what their siblings without history queue -- ``max_iter`` rounds per chunk, of k_secant_history, and for the tangent
one launch of k_secant_tangent_history and one elimination on the sibling plan -- and read nothing back: on a non-blocking stream
behind inputs that are still in flight, the history among them, they must give, bit for bit, what the same call gives on the null
stream with everything synchronised.  The file sorts behind test_gpu_stream_order.py and the secant files (the shared
plans of stream_order_gpu.py keep their scratch grown from one file to the next).

The law is that of test_gpu_stream_order_secant.py with every entry scaled by 1 / (1 + h0 / 8) more, and the update of h0 is the
largest of h0 and |e|: every input the entries read (coef, M, xi, rows, history) reaches every floating-point output.  It reads no s.
"""

import numpy as np
import pytest

import stream_order_gpu as H
from test_gpu_stream_order import CELLS, DELAY_MS
from test_gpu_stream_order_secant import PLANS, ROUNDS
from test_gpu_stream_order_secant import _inputs as _secant_inputs
from test_gpu_stream_order_secant_tangent import _sibling

pytestmark = pytest.mark.gpu

_cache = {}


def _law(p):
    from hommx_amd.expr import SecantLaw

    soft = "(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))/(1 + 0.125*h[0])"
    texts = [f"c[{k}]*{soft}" + (" + 0.015625*abs(x[0])*c[0]" if k == 0 else "") for k in range(p.n_comp)]
    update = ["max(h[0], sqrt(e[0]**2 + e[1]**2))"]
    return SecantLaw(texts[0], history=update) if p.n_comp == 1 else SecantLaw(lam=texts[0], mu=texts[1], history=update)


def _inputs(name, nc, seed):
    d = dict(_secant_inputs(name, nc, seed))
    d["history"] = np.random.default_rng(177 + seed).integers(0, 9, (nc, H.plan(name).n_el, 1)) / 8.0
    return d


def _outputs(p, nc):
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    return dict(H._tensor_outputs(p, nc), state=((nc, 3), H.F64), mean_flux=((nc, p.t), H.F64), coef_out=((nc,) + el, H.F64),
                history_out=((nc, p.n_el, 1), H.F64))


NAMES = ("coef", "M", "xi", "rows", "history")


def call_secant_history(name, p, nc, real, decoy):
    law = _law(p)
    return H.Call("secant_history", p, real, decoy, NAMES, _outputs(p, nc),
                  lambda a, st: p.secant_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, a["rows"], a["state"], a["A_eff"],
                                                max_iter=ROUNDS, tol=0.0, mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"],
                                                info_ptr=a["info"], stream=st, history_in_ptr=a["history"],
                                                history_out_ptr=a["history_out"]))


def call_secant_tangent_history(name, p, nc, real, decoy):
    out = dict(_outputs(p, nc), tangent=((nc, p.t, p.t), H.F64), asymmetry=((nc,), H.F64),
               tangent_coef=((nc, p.n_el, p.t * (p.t + 1) // 2), H.F64))
    law, sib = _law(p), _sibling(name)
    return H.Call("secant_tangent_history", p, real, decoy, NAMES, out,
                  lambda a, st: p.secant_tangent_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, sib, a["rows"], a["state"],
                                                        a["A_eff"], a["tangent"], a["asymmetry"], max_iter=ROUNDS, tol=0.0,
                                                        mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"], info_ptr=a["info"],
                                                        tangent_coef_ptr=a["tangent_coef"], stream=st, history_in_ptr=a["history"],
                                                        history_out_ptr=a["history_out"]))


CALLS = {"secant": call_secant_history, "tangent": call_secant_tangent_history}


def _case(which, name):
    if (which, name) not in _cache:
        nc = CELLS[name]
        call = CALLS[which](name, H.plan(name), nc, _inputs(name, nc, 1), _inputs(name, nc, 2))
        _cache[which, name] = (call,) + H.references(call)
    return _cache[which, name]


@pytest.mark.parametrize("name", PLANS)
@pytest.mark.parametrize("which", list(CALLS))
def test_history_device_entries_in_flight(which, name):
    call, real, _ = _case(which, name)
    assert np.array_equal(real["state"][:, 0], np.full(CELLS[name], ROUNDS)) and np.array_equal(real["state"][:, 2], np.ones(CELLS[name]))
    assert not np.array_equal(real["history_out"], _inputs(name, CELLS[name], 1)["history"])  # some element has loaded
    H.in_flight(call, real, DELAY_MS)


def test_null_stream_calls_equal_the_host_entries():
    name = "small_wave"
    p, d = H.plan(name), _inputs(name, CELLS[name], 1)
    kw = dict(rows=d["rows"], max_iter=ROUNDS, tol=0.0, return_coef=True, history=d["history"])
    _, real, _ = _case("secant", name)
    r = p.secant(d["coef"], d["xi"], _law(p), d["M"], **kw)
    assert np.array_equal(real["state"], np.stack([r.rounds, r.change, r.status], axis=1).astype(np.float64))
    for k, a in (("A_eff", r.A_eff), ("mean_flux", r.mean_flux), ("coef_out", r.coef), ("info", r.info), ("history_out", r.history)):
        assert np.array_equal(real[k], a), k
    _, real, _ = _case("tangent", name)
    r = p.secant_tangent(d["coef"], d["xi"], _law(p), _sibling(name), d["M"], return_tangent_coef=True, **kw)
    for k, a in (("A_eff", r.A_eff), ("mean_flux", r.mean_flux), ("coef_out", r.coef), ("info", r.info), ("history_out", r.history),
                 ("tangent", r.tangent), ("asymmetry", r.asymmetry), ("tangent_coef", r.tangent_coef)):
        assert np.array_equal(real[k], a), k
