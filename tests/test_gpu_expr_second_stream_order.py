"""The stream-order contract of the device entries that form second-order tangents (-m gpu), under the in-flight protocol of
tests/stream_order_gpu.py: hommx_expand_second_tangents_device writes straight into the caller's arrays (three launches for the three
slots here), and hommx_second_sensitivity_source_device with HOMMX_DIRS_PARAMETERS_CURVATURE expands the chunk's stream, tangents and
second-order streams into plan scratch (B_EXPAND, B_TANGENT, B_CURVATURE) and adds the curvature term, all on the caller's stream.
Every call runs on a non-blocking stream behind inputs still in flight and must equal, bit for bit, the same call on the null stream
with everything synchronised.  The expression is positive for every midpoint in [0, 1]^3, so a premature or late read gives wrong
numbers, never a pivot failure."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELAY_MS = 100.0  # that of test_gpu_stream_order.py and test_gpu_expr_params_stream_order.py
NC = 40


def _call(entry):
    import stream_order_gpu as H
    from hommx_amd import _lib, hmm, mesh as Mm
    from hommx_amd.batch import Program

    p = H.plan("fused2d_16")
    A = hmm.Expression("1.5 + x[0] + p[0]**2*y[0]*y[1] + p[1]*sin(2*pi*y[0] + x[1])*p[0] + (p[2] + p[1])**2*x[2]", p=[0.75, 0.25, 0.5])
    ops, consts = A.program()
    prog = Program(ops, consts, 1, A.n_params)
    bary, w = hmm.micro_quadrature(2, A.degree)
    yq = np.ascontiguousarray(np.einsum("qa,eak->eqk", bary, Mm.create_unit_square(5, 5).cell_vertices()))
    sets = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        sets.append({"points": yq, "weights": np.ascontiguousarray(w), "mid": rng.uniform(0.0, 1.0, (NC, 3)),
                     "M": np.eye(2)[None] + 0.2 * rng.uniform(-1.0, 1.0, (NC, 2, 2))})
    struct = prog.struct()

    def source(a):
        return _lib.CoefSource(form=_lib.COEF_PROGRAM, n_q=len(w), table=a["points"], weights=a["weights"], params=a["mid"], program=C.pointer(struct))

    nd, t = A.n_params, p.t
    if entry == "expand_second_tangents":
        out = {"coef": ((NC, p.n_el), H.F64), "dirs": ((NC, nd, p.n_el), H.F64), "curv": ((NC, nd * (nd + 1) // 2, p.n_el), H.F64)}
        invoke = lambda a, st: p.expand_second_tangents_device(NC, source(a), a["coef"], a["dirs"], a["curv"], st)
        names = ("points", "weights", "mid")
    else:
        out = dict(H._tensor_outputs(p, NC), d2A=((NC, nd, nd, t, t), H.F64), dA=((NC, nd, t, t), H.F64))
        invoke = lambda a, st: p.second_sensitivities_device(NC, source(a), a["M"], nd, None, a["d2A"], "parameters", a["dA"], a["A_eff"], a["info"], st,
                                                             curvature=True)
        names = ("points", "weights", "mid", "M")
    call = H.Call(entry + "_curvature", p, sets[0], sets[1], names, out, invoke)
    call.keep = (prog, struct)
    return H, call


@pytest.mark.parametrize("entry", ["expand_second_tangents", "second_sensitivities"])
def test_in_flight(entry):
    H, call = _call(entry)
    real, _ = H.references(call)  # also grows every scratch the call needs
    H.in_flight(call, real, DELAY_MS)
