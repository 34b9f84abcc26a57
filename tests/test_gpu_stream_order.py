"""The stream-order contract of every `*_device` entry point on an MI355X (-m gpu): "asynchronous on `stream`" (include/hommx_hip.h,
hommx_solve_batch_device) under the in-flight protocol of tests/stream_order_gpu.py.  Every call runs on a non-blocking stream behind
inputs that are still in flight (held back by one bounded spin), with its outputs taken and its inputs overwritten in stream order right
behind it, and must equal, bit for bit, the same call on the null stream with everything synchronised.  Accuracy is pinned elsewhere;
this file pins ordering: the fork / join of mf_solve's side streams, the expansion of sampler forms into plan scratch, the corrector
scratch reused chunk after chunk, scratch regrown in the middle of a queue, and two plans side by side.

The delay.  Wall time of the synchronous reference calls on an MI355X, launch through synchronise, in ms; "first" is a case's first
call, which also grows scratch and loads code, "warm" its second (the decoy's), which is what the call in flight repeats:

    entry                 fused2d_16  fused2d_32  small_wave  small_fused  multifrontal  mesh_front  mesh_tree     (first / warm)
    solve                 0.43/0.03   0.14/0.12   2.93/0.06   2.47/0.25    3.47/0.47     1.51/0.39   2.80/0.25
    solve, 520 cells                                                       2.00/1.19
    solve, M = None                   0.93/0.11
    two_phase                         0.14/0.12   0.12/0.05                0.55/0.48
    separable (affine)                0.14/0.12   0.10/0.05                0.53/0.49
    separable (reciprocal)            0.16/0.14
    reconstruct                       2.46/0.17   1.93/0.41                2.52/0.71     0.79/0.58   1.60/0.28
    reconstruct_source                0.23/0.18   0.45/0.43                0.80/0.74     0.69/0.58   0.37/0.30
    sensitivities                     1.15/0.18   0.43/0.37                0.85/0.82     0.64/0.58   0.33/0.28
    stratification                    1.45/0.19   0.44/0.37                0.94/0.90     0.66/0.58   0.35/0.30
    loads                             2.81/0.24   0.81/0.72                1.86/1.67     0.64/0.57   0.65/0.57
    first call of a 1 MB plan         0.62 (20 cells)                      3.22 (70 cells)

The largest is 3.47 ms (1.67 ms warm); four times that is 14 ms.  A first call that also loads the library's code has been seen to take
20 ms (the 40-cell multifrontal solve, in another process), and four times that is 80 ms: DELAY_MS rounds up to 100 ms.  Behind that delay
the host queues the staging copies and the library call in 0.3 to 6 ms (stream_order_gpu.in_flight prints it), so `ready` is asked about
with more than 90 ms to spare.  The 520-cell case takes no longer than the others (0.13 s, delay included); the whole file runs in about 10 s.

That the protocol has teeth was checked once against three deliberately mis-ordered builds of the library (not committed): mf_solve
without the caller's stream waiting for the pieces, mf_solve without the side streams waiting for the fork event, and the two-phase
expansion launched on the null stream.  16, 18 and 9 of the cases that reach that code failed; test_protocol_sees_a_call_that_does_not_wait
is the committed stand-in for those runs.
"""

import math

import numpy as np
import pytest
import torch

import stream_order_gpu as H

pytestmark = pytest.mark.gpu

DELAY_MS = 100.0  # the module docstring derives it

# plan -> cells.  mf_solve (multifrontal.hip) forks a chunk of `step_cells` cells onto plan-owned side streams when step_cells >= 16, into
# max(2, min(4, nc / 128)) pieces: 40 cells run as two pieces (one side stream), 520 cells (520 / 128 = 4) as four (all three side
# streams).  A change of that rule must change these counts.
CELLS = {"fused2d_16": 24, "fused2d_32": 24, "small_wave": 24, "small_fused": 24, "multifrontal": 40, "mesh_front": 24, "mesh_tree": 40}
MF4_CELLS = 520
assert CELLS["multifrontal"] >= 16 and CELLS["multifrontal"] // 128 < 2 and CELLS["mesh_tree"] >= 16 and MF4_CELLS // 128 == 4
DERIVED = ["fused2d_32", "small_wave", "multifrontal", "mesh_front", "mesh_tree"]
SAMPLED = ["fused2d_32", "small_wave", "multifrontal"]
ENTRIES = {
    "solve": H.call_solve,
    "solve_no_M": lambda p, nc, r, d: H.call_solve(p, nc, r, d, with_M=False, label="solve_no_M"),
    "two_phase": H.call_two_phase,
    "affine": lambda p, nc, r, d: H.call_separable(p, nc, r, d, "affine"),
    "reciprocal": lambda p, nc, r, d: H.call_separable(p, nc, r, d, "reciprocal"),
    "reconstruct": H.call_reconstruct,
    "reconstruct_source": H.call_reconstruct_source,
    "sensitivities": H.call_sensitivities,
    "sensitivities_two_phase": lambda p, nc, r, d: H.call_sensitivities(p, nc, r, d, form="two_phase"),
    "stratification": H.call_strat,
    "loads": H.call_loads,
    "loads_P_eff": lambda p, nc, r, d: H.call_loads(p, nc, r, d, response=False),
}
_cache = {}


def _call(name, entry, nc, p=None, seeds=(1, 2)):
    """The Call of ENTRIES[entry] for `nc` cells of plan `name` (on `p`: another plan of that shape)."""
    return ENTRIES[entry](p or H.plan(name), nc, H.inputs(name, nc, seeds[0]), H.inputs(name, nc, seeds[1]))


def _case(name, entry, nc=None):
    """(call, reference of the real inputs, reference of the decoy) on the shared plan of `name`: computed once, read only."""
    key = (name, entry, nc or CELLS[name])
    if key not in _cache:
        call = _call(name, entry, key[2])
        _cache[key] = (call,) + H.references(call)
    return _cache[key]


def _run(name, entry, nc=None):
    call, real, _ = _case(name, entry, nc)
    H.in_flight(call, real, DELAY_MS)


# -- the entry points, one call in flight ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CELLS))
def test_solve_device(name):
    _run(name, "solve")


def test_solve_device_four_pieces():
    """520 cells of the multifrontal plan: the only case that reaches four pieces, all three side streams."""
    _run("multifrontal", "solve", MF4_CELLS)


def test_solve_device_unstratified():
    """M = None on a fused 2D plan: the unstratified kernel."""
    _run("fused2d_32", "solve_no_M")


@pytest.mark.parametrize("name,form", [(n, f) for n in SAMPLED for f in ("two_phase", "affine")] + [("fused2d_32", "reciprocal")])
def test_sampler_solves(name, form):
    """On the multifrontal plan the form is expanded into plan scratch on the caller's stream, and side streams then read that scratch."""
    _run(name, form)


@pytest.mark.parametrize("name", DERIVED)
def test_reconstruct_device(name):
    _run(name, "reconstruct")


@pytest.mark.parametrize("name", DERIVED)
def test_reconstruct_source_device(name):
    _run(name, "reconstruct_source")


@pytest.mark.parametrize("name", DERIVED)
def test_sensitivities_device(name):
    _run(name, "sensitivities")


@pytest.mark.parametrize("name", DERIVED)
def test_stratification_sensitivities_device(name):
    _run(name, "stratification")


@pytest.mark.parametrize("name", DERIVED)
def test_loads_device(name):
    """The response and the load correctors; the frontal mesh route refuses the response: P_eff alone there."""
    _run(name, "loads_P_eff" if name == "mesh_front" else "loads")


# -- the protocol notices a call that does not wait for its inputs -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused2d_32", "multifrontal", "mesh_front"])
def test_protocol_sees_a_call_that_does_not_wait(name):
    call, real, decoy = _case(name, "solve")
    H.unordered(call, real, decoy, DELAY_MS)


# -- chunked in flight -------------------------------------------------------------------------------------------------------------------
# bytes per cell of recon_chunk (api.hip): the correctors, t vectors of ndof doubles (both plans' ndof fit the LDS: no chi^xi slot), and
# the factor record of a fused 2D plan (kernels.h, fused_fact_doubles: header 4 NB + 8, n - 1 steps of NB^2 + 4 NB, the last block NB^2)
#   multifrontal  3D elasticity n = 5: 6 x 375 x 8 = 18,000 B                    -> 1 MiB holds 58 cells: 70 cells run as 58 + 12, both >= 12 ...
#   fused2d_32    n = 17, NB = 32: 2 x 289 x 8 + (136 + 16 x 1152 + 1024) x 8 = 161,360 B -> 6 cells: 20 cells run as 6 + 6 + 6 + 2
# ... and the first multifrontal chunk, 58 >= 16 cells, forks.
CHUNKED = {"multifrontal": (70, 6 * 375 * 8, 2), "fused2d_32": (20, 2 * 289 * 8 + (136 + 16 * 1152 + 1024) * 8, 4)}


@pytest.mark.parametrize("name", list(CHUNKED))
@pytest.mark.parametrize("entry", ["reconstruct_source", "sensitivities_two_phase"])
def test_chunked_in_flight(name, entry, monkeypatch):
    """HOMMX_RECON_MEM_MB is read when a plan is created: a fresh plan runs the batch in chunks of 1 MB, every chunk through the same
    corrector scratch and expanded stream.  The reference comes from the default plan: chunking does not change a bit."""
    nc, per_cell, chunks = CHUNKED[name]
    assert math.ceil(nc / ((1 << 20) // per_cell)) == chunks and chunks >= (3 if name == "fused2d_32" else 2)
    _, real, _ = _case(name, entry, nc)
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")
    p = H.new_plan(name)
    monkeypatch.undo()
    call = _call(name, entry, nc, p)
    warm = H.reference(call, 0)  # grows the chunked plan's scratch
    for k, a in real.items():
        assert np.array_equal(warm[k], a), k
    H.in_flight(call, real, DELAY_MS)
    p.close()


# -- a queue without host synchronisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multifrontal", "fused2d_32"])
def test_queue_regrows_scratch(name):
    """Four calls of growing size on one fresh plan, queued behind one delay with nothing but stream order between them: scratch is
    regrown while earlier calls are still queued.  `ready` is not asked about here: a regrow may legitimately block the host."""
    queue = [("solve", 8), ("reconstruct", 40), ("sensitivities", 24), ("solve", 40)]
    refs = [_case(name, entry, nc)[1] for entry, nc in queue]  # the shared plan of this shape, warmed
    p = H.new_plan(name)
    flights = [H.Flight(_call(name, entry, nc, p)) for entry, nc in queue]
    s = torch.cuda.Stream(flights[0].dev)
    H.delay(s, DELAY_MS)
    for f in flights:
        f.stage(s)
        f.launch(s)
        f.collect(s)
    s.synchronize()
    for f, want in zip(flights, refs):
        f.check(want)
    p.close()


# -- two plans, two streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["multifrontal", "fused2d_32"])
def test_two_plans_on_two_streams(other):
    """"Distinct plans are independent": a multifrontal plan on s1 and a second plan with other data on s2, each behind its own delay,
    the host calls interleaved, each against its own reference."""
    p2 = H.new_plan(other)
    pairs = []
    for entry in ("solve", "reconstruct"):
        a, want_a, _ = _case("multifrontal", entry)
        b = _call(other, entry, CELLS[other], p2, seeds=(3, 4))
        pairs.append((H.Flight(a), want_a, H.Flight(b), H.references(b)[0]))
    dev = pairs[0][0].dev
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    H.delay(s1, DELAY_MS)
    H.delay(s2, DELAY_MS)
    pending = []
    for fa, _, fb, _ in pairs:
        fa.stage(s1)
        fb.stage(s2)
        fa.launch(s1)
        fb.launch(s2)
        pending += [not fa.ready.query(), not fb.ready.query()]
        fa.collect(s1)
        fb.collect(s2)
    s1.synchronize()
    s2.synchronize()
    assert all(pending), pending
    for fa, want_a, fb, want_b in pairs:
        fa.check(want_a)
        fb.check(want_b)
    p2.close()
