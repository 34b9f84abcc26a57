"""Helpers of tests/test_gpu_stream_order.py: the plans, two valid input sets per plan, the device entry points as ``Call`` objects, and the
in-flight protocol that pins "asynchronous on `stream`" (include/hommx_hip.h, hommx_solve_batch_device).

The protocol, for one ``Call`` (a plan, an entry point, a real and a decoy input set):

  reference   the entry on the null stream with blocking uploads and a device synchronise, for the real and for the decoy inputs: the
              configuration the rest of the suite trusts.  It also grows every plan scratch the call needs.
  buffers     every device input the entry reads is a persistent tensor that holds the DECOY; the real values wait in staging tensors.
              Every output buffer holds NaN (info: -7).
  in flight   on a non-blocking stream s, with no host synchronisation in between: a bounded spin (torch.cuda._sleep), the real inputs
              copied over the decoys, event `ready`, the library call, every output copied to a "kept" tensor, the decoys copied back over
              the inputs, NaN over the outputs.
  checks      `ready` is still unset when the call has returned (the inputs had not landed: the run proved something), and after
              s.synchronize() every kept output equals the reference bitwise.

Work that starts before the inputs are there reads the decoy (and so does anything launched on the null stream, which does not order
against s); work the caller's stream does not wait for leaves NaN in the kept copy; work that reads its inputs after control returned to
the stream reads the decoy written back.  Both input sets are valid (SPD coefficients, M near the identity, 0 / 1 masks, labels < 8, a + b g
> 0 for any mixture of the two sets), so a premature or late read gives wrong numbers, never a pivot failure or a fault.
"""

from __future__ import annotations

import functools
import time

import numpy as np
import torch

import recon_ref as R
from hommx_amd import MicroCellPlan, _lib, workloads as W

# name -> (dim, n or None on the jittered mesh of that dimension, kind, route of from_mesh, kernel of the plan's tensor route,
#          corrector route, route of the load solve)
PLANS = {
    "fused2d_16": (2, 5, "poisson", None, "fused2d", "fused2d_subst", "fused2d_subst"),  # NB = 16
    "fused2d_32": (2, 17, "poisson", None, "fused2d", "fused2d_subst", "fused2d_subst"),  # NB = 32, padded
    "small_wave": (2, 4, "elasticity", None, "small_wave", "blocked", "blocked"),  # correctors: the plane elimination
    "small_fused": (3, 8, "poisson", None, "small_fused", "blocked", "blocked"),  # LDS kernel
    "multifrontal": (3, 5, "elasticity", None, "multifrontal", "multifrontal", "multifrontal"),  # the mf and the mf_keep plan
    "mesh_front": (2, None, "elasticity", "front", "mesh_front", "mesh_front", "none"),
    "mesh_tree": (3, None, "poisson", "tree", "mesh_multifrontal", "mesh_multifrontal", "mesh_multifrontal"),
}
WQ = 4  # quadrature points of the reciprocal sampler's table


@functools.lru_cache(maxsize=None)
def mesh(dim: int):
    return W.jittered_unit_square(9, 7) if dim == 2 else W.jittered_unit_cube(3, 4, 3)


def new_plan(name: str) -> MicroCellPlan:
    """A fresh plan of PLANS[name] (scratch not grown), its three routes asserted."""
    dim, n, kind, route, kernel, corrector, load = PLANS[name]
    p = MicroCellPlan(dim, n, kind) if n else MicroCellPlan.from_mesh(mesh(dim), kind, route=route)
    assert (p.kernel, p.corrector_kernel, p.load_kernel) == (kernel, corrector, load), (name, p.kernel, p.corrector_kernel, p.load_kernel)
    return p


@functools.lru_cache(maxsize=None)
def plan(name: str) -> MicroCellPlan:
    """The shared plan of PLANS[name]: its scratch stays grown from one case to the next."""
    return new_plan(name)


@functools.lru_cache(maxsize=None)
def inputs(name: str, nc: int, seed: int) -> dict:
    """One valid input set of every entry point for `nc` cells of PLANS[name], read only.  Coefficients as recon_ref.random_coef /
    random_M draw them, contrast 1e2; two shared directions; t shared loads; labels in {0, 1, 2}; a in [2, 3], b in [0.2, 0.8] and
    |g| <= 1, so a + b g > 0 whichever set each of them comes from."""
    dim, _, kind, *_ = PLANS[name]
    p = plan(name)
    rng = np.random.default_rng(1000 * seed + sorted(PLANS).index(name))
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    lead = (nc,) + ((p.n_comp,) if p.n_comp > 1 else ())
    d = {
        "coef": np.stack([R.random_coef(kind, dim, p.n_el, rng) for _ in range(nc)]),
        "M": np.stack([R.random_M(dim, rng) for _ in range(nc)]),
        "xi": rng.standard_normal((nc, p.t)),
        "dirs": rng.standard_normal((2,) + el),
        "w": rng.standard_normal((nc, p.t, p.t)),
        "P": rng.standard_normal((p.t, p.n_el, p.t)),
        "region": rng.integers(0, 3, p.n_el).astype(np.uint8),
        "mask": (rng.random(p.n_el) < 0.4).astype(np.uint8),
        "values": np.stack([R.random_coef(kind, dim, 2, rng) for _ in range(nc)]),  # two "elements": the two phases of a cell
        "table": rng.uniform(-1.0, 1.0, p.n_el),
        "table_q": rng.uniform(-1.0, 1.0, (p.n_el, WQ)),
        "wq": rng.dirichlet(np.ones(WQ)),
        "params": np.stack([rng.uniform(2.0, 3.0, lead), rng.uniform(0.2, 0.8, lead)], axis=-1),
    }
    for k, a in d.items():
        d[k] = np.ascontiguousarray(a)
        d[k].setflags(write=False)
    return d


class Call:
    """One device entry point on one plan: the inputs it reads (name -> (real, decoy)), the outputs it writes (name -> (shape, dtype)),
    and ``invoke(a, stream)``, which makes the library call with the device addresses a[name] (a.get(name): None when absent)."""

    def __init__(self, label: str, p: MicroCellPlan, real: dict, decoy: dict, names, outputs: dict, invoke):
        self.label, self.plan, self.invoke = label, p, invoke
        self.inputs = {k: (real[k], decoy[k]) for k in names}
        self.outputs = outputs


F64, I32 = np.float64, np.int32


def _source(a: dict, form: str) -> "_lib.CoefSource":
    src = _lib.CoefSource()
    if form == "sampled":
        src.form, src.coef = _lib.COEF_SAMPLED, a["coef"]
    else:
        src.form, src.mask, src.values = _lib.COEF_TWO_PHASE, a["mask"], a["values"]
    return src


def _tensor_outputs(p, nc):
    return {"A_eff": ((nc, p.t, p.t), F64), "info": ((nc,), I32)}


def call_solve(p, nc, real, decoy, with_M=True, label="solve"):
    names = ("coef", "M") if with_M else ("coef",)
    return Call(label, p, real, decoy, names, _tensor_outputs(p, nc),
                lambda a, st: p.solve_device(nc, a["coef"], a.get("M"), a["A_eff"], a["info"], st))


def call_two_phase(p, nc, real, decoy):
    return Call("two_phase", p, real, decoy, ("mask", "values", "M"), _tensor_outputs(p, nc),
                lambda a, st: p.solve_two_phase_device(nc, a["mask"], a["values"], a["M"], a["A_eff"], a["info"], st))


def call_separable(p, nc, real, decoy, family):
    if family == "affine":
        real, decoy, names, nq = real, decoy, ("table", "params", "M"), 1
    else:
        real, decoy = dict(real, table=real["table_q"]), dict(decoy, table=decoy["table_q"])
        names, nq = ("table", "wq", "params", "M"), WQ
    return Call("separable_" + family, p, real, decoy, names, _tensor_outputs(p, nc),
                lambda a, st: p.solve_separable_device(nc, family, nq, a["table"], a.get("wq"), a["params"], a["M"], a["A_eff"], a["info"], st))


def call_reconstruct(p, nc, real, decoy):
    out = dict(_tensor_outputs(p, nc), stats=((nc, 2 * p.t + 3), F64), strain=((nc, p.n_el, p.t), F64), flux=((nc, p.n_el, p.t), F64))
    return Call("reconstruct", p, real, decoy, ("coef", "M", "xi"), out,
                lambda a, st: p.reconstruct_device(nc, a["coef"], a["M"], a["xi"], a["stats"], a["strain"], a["flux"], a["A_eff"], a["info"], st))


def call_reconstruct_source(p, nc, real, decoy):
    """A two-phase source (expanded into plan scratch on the caller's stream) and two regions by explicit labels."""
    out = dict(_tensor_outputs(p, nc), stats=((nc, 2 * p.t + 3), F64), region_stats=((nc, 2, 2 * p.t + 4), F64))
    return Call("reconstruct_source", p, real, decoy, ("mask", "values", "M", "xi", "region"), out,
                lambda a, st: p.reconstruct_source_device(nc, _source(a, "two_phase"), a["M"], a["xi"], a["stats"], 2, a["region"],
                                                          a["region_stats"], None, None, a["A_eff"], a["info"], st))


def call_sensitivities(p, nc, real, decoy, form="sampled"):
    """Two shared directions, weights, the gradient asked for."""
    el = (p.n_el,) + ((p.n_comp,) if p.n_comp > 1 else ())
    out = dict(_tensor_outputs(p, nc), dA=((nc, 2, p.t, p.t), F64), grad=((nc,) + el, F64))
    names = (("coef",) if form == "sampled" else ("mask", "values")) + ("M", "dirs", "w")
    return Call("sensitivities", p, real, decoy, names, out,
                lambda a, st: p.sensitivities_device(nc, _source(a, form), a["M"], 2, a["dirs"], False, a["dA"], a["w"], a["grad"],
                                                     a["A_eff"], a["info"], st))


def call_strat(p, nc, real, decoy):
    """Weights and the full derivative."""
    out = dict(_tensor_outputs(p, nc), dA_dM=((nc, p.dim, p.dim, p.t, p.t), F64), grad_M=((nc, p.dim, p.dim), F64))
    return Call("stratification", p, real, decoy, ("coef", "M", "w"), out,
                lambda a, st: p.stratification_sensitivities_device(nc, _source(a, "sampled"), a["M"], a["dA_dM"], a["w"], a["grad_M"],
                                                                    a["A_eff"], a["info"], st))


def call_loads(p, nc, real, decoy, response=True):
    """t shared loads; with `response` the load solve: energy, stats and the load correctors."""
    bs = 1 if p.kind.startswith("poisson") else p.dim
    out = dict(_tensor_outputs(p, nc), P_eff=((nc, p.t, p.t), F64))
    if response:
        out.update(energy=((nc, p.t, p.t), F64), stats=((nc, p.t, p.t + 2), F64), correctors=((nc, p.t, p.n_nodes * bs), F64))
    return Call("loads", p, real, decoy, ("coef", "M", "P"), out,
                lambda a, st: p.loads_device(nc, _source(a, "sampled"), a["M"], p.t, a["P"], a["P_eff"], False, a["A_eff"], a["info"],
                                             a.get("energy"), a.get("stats"), None, None, a.get("correctors"), st))


# -- the delay ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cycles_per_ms(device: int) -> float:
    """Cycles of torch.cuda._sleep per millisecond on this device: two events around one short sleep, measured once."""
    dev = torch.device("cuda", device)
    s = torch.cuda.Stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        torch.cuda._sleep(100_000)  # the spin kernel's first launch loads its code
        e0.record()
        torch.cuda._sleep(2_000_000)
        e1.record()
    e1.synchronize()
    rate = 2_000_000 / e0.elapsed_time(e1)
    print(f"stream_order: {rate:.0f} cycles of torch.cuda._sleep per ms")
    return rate


def delay(s: "torch.cuda.Stream", ms: float):
    """One bounded spin of `ms` milliseconds (at most 500) queued on `s`."""
    assert 0 < ms <= 500.0
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(ms * cycles_per_ms(s.device.index)))


# -- the protocol ------------------------------------------------------------------------------------------------------------------------
def _nan(t: "torch.Tensor"):
    t.fill_(float("nan") if t.is_floating_point() else -7)


def reference(call: Call, which: int) -> dict:
    """The outputs of `call` on the null stream, fully synchronised, for its real (0) or decoy (1) inputs.  Prints the wall time of
    the call, launch through synchronise (module docstring of test_gpu_stream_order: the delay is sized on these)."""
    dev = torch.device("cuda", call.plan.device)
    ins = {k: torch.from_numpy(np.array(v[which])).to(dev) for k, v in call.inputs.items()}
    outs = {k: torch.empty(shape, dtype=torch.float64 if dt is F64 else torch.int32, device=dev) for k, (shape, dt) in call.outputs.items()}
    for t in outs.values():
        _nan(t)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    call.invoke({k: t.data_ptr() for k, t in {**ins, **outs}.items()}, None)
    torch.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0)
    print(f"stream_order: reference {call.label} of {call.plan.kernel}, {next(iter(call.outputs.values()))[0][0]} cells, "
          f"{'decoy' if which else 'real'} inputs: {ms:.2f} ms")
    got = {k: t.cpu().numpy() for k, t in outs.items()}
    for k, a in got.items():
        assert np.isfinite(a).all() and (k != "info" or not a.any()), (call.label, k)
    return got


def references(call: Call) -> tuple[dict, dict]:
    """(real, decoy) references; they must differ in every floating-point output, or the decoy would hide nothing."""
    real, decoy = reference(call, 0), reference(call, 1)
    for k in real:
        assert k == "info" or not np.array_equal(real[k], decoy[k]), (call.label, k)
    return real, decoy


class Flight:
    """The device buffers of one call in flight: persistent inputs holding the decoy, staging tensors, NaN outputs, kept copies."""

    def __init__(self, call: Call):
        self.call = call
        dev = self.dev = torch.device("cuda", call.plan.device)
        up = lambda a: torch.from_numpy(np.array(a)).to(dev)
        self.buf = {k: up(v[1]) for k, v in call.inputs.items()}
        self.real = {k: up(v[0]) for k, v in call.inputs.items()}
        self.decoy = {k: up(v[1]) for k, v in call.inputs.items()}
        self.out = {k: torch.empty(shape, dtype=torch.float64 if dt is F64 else torch.int32, device=dev) for k, (shape, dt) in call.outputs.items()}
        self.kept = {k: torch.empty_like(t) for k, t in self.out.items()}
        for t in list(self.out.values()) + list(self.kept.values()):
            _nan(t)
        self.ready = torch.cuda.Event()
        cycles_per_ms(dev.index)  # calibrated before anything is in flight
        torch.cuda.synchronize(dev)  # the fills ran on the null stream, which a non-blocking stream does not order against

    def stage(self, s):
        """On s: the real inputs over the decoys, then `ready`."""
        with torch.cuda.stream(s):
            for k, t in self.buf.items():
                t.copy_(self.real[k], non_blocking=True)
            self.ready.record(s)

    def launch(self, s):
        """The library call on s."""
        self.call.invoke({k: t.data_ptr() for k, t in {**self.buf, **self.out}.items()}, s.cuda_stream)

    def collect(self, s):
        """On s: every output to its kept tensor, the decoys back over the inputs, NaN over the outputs."""
        with torch.cuda.stream(s):
            for k, t in self.out.items():
                self.kept[k].copy_(t, non_blocking=True)
            for k, t in self.buf.items():
                t.copy_(self.decoy[k], non_blocking=True)
            for t in self.out.values():
                _nan(t)

    def results(self) -> dict:
        return {k: t.cpu().numpy() for k, t in self.kept.items()}

    def check(self, want: dict):
        got = self.results()
        for k, a in want.items():
            assert np.array_equal(got[k], a), (self.call.label, self.call.plan.kernel, k)


def in_flight(call: Call, want: dict, delay_ms: float, require_pending: bool = True) -> Flight:
    """The protocol for one call whose scratch is grown: everything queued on one non-blocking stream behind the delay, `ready` still
    unset when the call has returned, and every kept output bitwise equal to `want`."""
    f = Flight(call)
    s = torch.cuda.Stream(f.dev)
    t0 = time.perf_counter()
    delay(s, delay_ms)
    f.stage(s)
    f.launch(s)
    pending = not f.ready.query()
    host_ms = 1e3 * (time.perf_counter() - t0)
    f.collect(s)
    s.synchronize()
    print(f"stream_order: {call.label} of {call.plan.kernel} queued in {host_ms:.2f} ms of host time behind a delay of {delay_ms:.0f} ms")
    if require_pending:
        assert pending, f"{call.label}: the inputs had landed when the call returned -- the delay held nothing back, or the entry blocked the host"
    f.check(want)
    return f


def unordered(call: Call, real: dict, decoy: dict, delay_ms: float):
    """The self-check of the protocol: the inputs staged behind the delay on s, the call on a SECOND stream with no event between the
    two.  That call does not wait for its inputs, so it must see the decoy: the harness notices such a call."""
    f = Flight(call)
    s, s2 = torch.cuda.Stream(f.dev), torch.cuda.Stream(f.dev)
    delay(s, delay_ms)
    f.stage(s)
    f.launch(s2)
    s2.synchronize()
    assert not f.ready.query(), f"{call.label}: the delay ran out before the unordered call had finished"
    got = {k: t.cpu().numpy() for k, t in f.out.items()}  # a blocking copy on the null stream: s2 is idle, s does not order against it
    s.synchronize()
    for k, a in decoy.items():
        assert np.array_equal(got[k], a), (call.label, k)
    assert any(not np.array_equal(got[k], a) for k, a in real.items()), call.label
