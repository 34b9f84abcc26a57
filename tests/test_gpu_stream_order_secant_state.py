"""The stream-order contract of hommx_secant_state_source_device on an MI355X (-m gpu) under the in-flight protocol of
tests/stream_order_gpu.py, on a fused plan, a blocked plan and a frontal mesh plan created with ``load_solve=True``.  The entry queues
``max_iter`` rounds per chunk and behind them the tail -- one launch of k_criterion_state on the blocks of the last round beside an
eigenstrain, or one launch of k_recon without a load -- and reads nothing back: on a non-blocking stream behind inputs that are still
in flight, the criterion's own rows among them, it must give, bit for bit, what the same call gives on the null stream with everything
synchronised.  The file sorts behind test_gpu_stream_order_secant_load.py (the shared plans of stream_order_gpu.py keep
their scratch grown from one file to the next) and creates no stream outside the protocol.

The law and the load are those of test_gpu_stream_order_secant_load.py; the criterion reads the total flux, the stopped stream, the
base stream and its own field, so every input the entry reads reaches its four statistics.
"""

import numpy as np
import pytest

import stream_order_gpu as H
from test_gpu_stream_order import CELLS, DELAY_MS
from test_gpu_stream_order_secant import ROUNDS, _law
from test_gpu_stream_order_secant_load import PLANS, _inputs as _load_inputs, _outputs, _plan

pytestmark = pytest.mark.gpu

_cache = {}


def _crit():
    from hommx_amd.expr import Criterion

    return Criterion("sqrt(s[0]**2 + s[1]**2)*f[0]/b[0] + c[0] + x[0]", fields=1, threshold=2.0)


def _inputs(name, nc, seed):
    d = dict(_load_inputs(name, nc, seed))
    d["crit_rows"] = np.random.default_rng(311 + seed).integers(1, 9, (nc, 4)) / 8.0
    return d


def call_criterion_tail(name, p, nc, real, decoy):
    law, crit = _law(p), _crit()
    out = dict(_outputs(p, nc), crit=((nc, 4), H.F64), values=((nc, p.n_el), H.F64), total_strain=((nc, p.n_el, p.t), H.F64),
               total_flux=((nc, p.n_el, p.t), H.F64))
    return H.Call("secant_state_criterion", p, real, decoy, ("coef", "M", "xi", "rows", "E", "crit_rows"), out,
                  lambda a, st: p.secant_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, a["rows"], a["state"], a["A_eff"],
                                                max_iter=ROUNDS, tol=0.0, mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"],
                                                info_ptr=a["info"], stream=st, P_ptr=a["E"], eigenstrain=True, criterion=crit,
                                                crit_rows_ptr=a["crit_rows"], crit_ptr=a["crit"], crit_values_ptr=a["values"],
                                                total_strain_ptr=a["total_strain"], total_flux_ptr=a["total_flux"]))


def call_reconstruction_tail(name, p, nc, real, decoy):
    law = _law(p)
    out = dict(_outputs(p, nc), stats=((nc, 2 * p.t + 3), H.F64))
    return H.Call("secant_state_reconstruct", p, real, decoy, ("coef", "M", "xi", "rows"), out,
                  lambda a, st: p.secant_device(nc, H._source(a, "sampled"), a["M"], a["xi"], law, a["rows"], a["state"], a["A_eff"],
                                                max_iter=ROUNDS, tol=0.0, mean_flux_ptr=a["mean_flux"], coef_ptr=a["coef_out"],
                                                info_ptr=a["info"], stream=st, stats_ptr=a["stats"]))


CALLS = {"criterion": call_criterion_tail, "reconstruct": call_reconstruction_tail}


def _case(which, name):
    if (which, name) not in _cache:
        nc = CELLS[name]
        call = CALLS[which](name, _plan(name), nc, _inputs(name, nc, 1), _inputs(name, nc, 2))
        _cache[which, name] = (call,) + H.references(call)
    return _cache[which, name]


@pytest.mark.parametrize("name", list(PLANS))
@pytest.mark.parametrize("which", list(CALLS))
def test_state_device_entry_in_flight(which, name):
    call, real, _ = _case(which, name)
    assert np.array_equal(real["state"][:, 0], np.full(CELLS[name], ROUNDS)) and np.array_equal(real["state"][:, 2], np.ones(CELLS[name]))
    H.in_flight(call, real, DELAY_MS)


def test_null_stream_calls_equal_the_host_entry():
    name = "fused2d_32"
    p, d = _plan(name), _inputs(name, CELLS[name], 1)
    _, real, _ = _case("criterion", name)
    r = p.secant(d["coef"], d["xi"], _law(p), d["M"], rows=d["rows"], max_iter=ROUNDS, tol=0.0, return_coef=True, P=d["E"], eigenstrain=True,
                 criterion=_crit(), crit_rows=d["crit_rows"], crit_values=True, crit_fields=True)
    c = r.criterion
    assert np.array_equal(real["crit"], np.stack([c.max, c.argmax_element.astype(np.float64), c.mean, c.exceed_volume], axis=1))
    for k, a in (("A_eff", r.A_eff), ("coef_out", r.coef), ("values", c.values), ("total_strain", c.strain), ("total_flux", c.flux)):
        assert np.array_equal(real[k], a), k
    _, real, _ = _case("reconstruct", name)
    r = p.secant(d["coef"], d["xi"], _law(p), d["M"], rows=d["rows"], max_iter=ROUNDS, tol=0.0, reconstruct=True).reconstruction
    assert np.array_equal(real["stats"][:, :p.t], r.mean_strain) and np.array_equal(real["stats"][:, 2 * p.t], r.energy)
