"""Criteria and reconstruction statistics of the nonlinear state on the device (-m gpu; k_criterion_state of csrc/criterion_state.hip,
hommx_secant_state_source), on the six shapes of test_gpu_elem_walk_bits.py, three seeded cells each, with and without M:
every (DIM, KIND, MESH) class of the kernel.  Held, every comparison bit for bit:

a. a criterion that reads neither ``b`` nor ``h``: statistics, values, strain and flux are those of
   ``plan.criterion(result.coef, xi, crit, ..., fields=True, values=True)`` -- without a load, beside a per-cell polarisation and beside
   a per-cell eigenstrain; the reconstruction tail is ``plan.reconstruct(result.coef, xi, M, regions=...)`` with three regions and one
   label >= 8; every secant output is the one of the call without a tail;
b. a criterion of exactly rounded operations that reads x y f e s c b h: ``values`` is ``host_values`` of the call's own total strain,
   total flux, ``coef``, base and ``history`` -- the contract test_gpu_criterion.py holds k_criterion to; ``b[20]`` on the Voigt mesh;
c. the slot path: 2D Poisson n = 112 at depth 16 beside the LDS path, one cell each, against ``host_values``;
d. chunking (360 cells through 1 MB chunks), batch position, ``max_iter`` beyond the stopping round, which tail outputs are asked for
   and the entry (host against device on the current stream) change nothing, on a fused plan, a blocked plan and a frontal mesh plan
   created with the load solve;
e. a cell stopped with status 1 is evaluated on its c^1; a cell of status 2 and a cell of status 3 leave the other cells' tail alone
   (the inputs of test_gpu_secant.py for the two statuses: they end in a status, not in a fault);
f. the solver classes end to end.

No stream is created here (DESIGN 4.15 records why): the device entry runs on the current stream.
"""

import numpy as np
import pytest

from test_gpu_criterion import EXACT
from test_gpu_elem_walk_bits import NC, SHAPES
from test_gpu_secant import CASES, _bits, _case, _law, _plan, soft_law
from test_gpu_secant_history import G, KAPPA, _history
from test_gpu_secant_load import _load

pytestmark = pytest.mark.gpu

LOADS = [None, False, True]  # no load, a polarisation, an eigenstrain
LOAD_IDS = ["plain", "P", "E"]
UPDATE = "max(h[0], abs(e[0]))"


def _crit(text, **kw):
    from hommx_amd.expr import Criterion

    return Criterion(text, **kw)


def _stats(c):
    return [c.max, c.argmax_element, c.mean, c.exceed_volume]


def _tail_bits(c):
    return _stats(c) + [c.values, c.strain, c.flux]


def _equal(got, want, what, cells=slice(None)):
    for k, (x, y) in enumerate(zip(got, want)):
        if x is not None and y is not None:
            assert np.array_equal(x[cells], y[cells], equal_nan=x.dtype.kind == "f"), f"{what}: item {k}"


def _secant(p, d, law, load=None, eigenstrain=False, **kw):
    rows = d["rows"][:, :3 + law.n_fields]
    if load is not None:
        kw.update(P=load, eigenstrain=eigenstrain)
    return p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, points=d["points"], **kw)


def _labels(p):
    """Three regions, and elements of no region: one label at or above 8 among them."""
    lab = np.arange(p.n_el) % 5
    lab[lab == 3] = 9
    lab[lab == 4] = 200
    return lab


# -- a. a criterion of the linear grammar, and the reconstruction ---------------------------------------------------------------------------
@pytest.mark.parametrize("eigenstrain", LOADS, ids=LOAD_IDS)
@pytest.mark.parametrize("shape,with_M", CASES)
def test_a_tail_without_b_and_h_is_the_criterion_on_coef_out(shape, with_M, eigenstrain):
    p, d = _case(shape, with_M)
    law = soft_law(p.kind, p.dim)
    crit = _crit(EXACT, p=[0.75], fields=1, threshold=0.5)
    load = None if eigenstrain is None else _load(shape, with_M)
    kw = dict(max_iter=3, tol=0.0, fields=True, values=True, return_coef=True)
    plain = _secant(p, d, law, load, bool(eigenstrain), **kw)
    r = _secant(p, d, law, load, bool(eigenstrain), criterion=crit, crit_rows=d["rows"][:, :4], crit_values=True, crit_fields=True, **kw)
    assert np.array_equal(r.status, np.ones(NC, dtype=np.int64)) and not r.info.any() and not np.array_equal(r.coef, d["coef"])
    _equal(_bits(r) + [r.strain, r.flux, r.values], _bits(plain) + [plain.strain, plain.flux, plain.values], "the secant outputs")
    want = p.criterion(r.coef, d["xi"], crit, d["M"], rows=d["rows"][:, :4], points=d["points"], values=True, fields=True, P=load,
                       eigenstrain=bool(eigenstrain))
    _equal(_tail_bits(r.criterion), _tail_bits(want), "the criterion")
    assert r.reconstruction is None and r.criterion.values.shape == (NC, p.n_el)
    assert np.array_equal(r.criterion.A_eff, r.A_eff)
    if eigenstrain is None:  # what the law read is what the criterion sees
        assert np.array_equal(r.criterion.strain, r.strain) and np.array_equal(r.criterion.flux, r.flux)


@pytest.mark.parametrize("shape,with_M", CASES)
def test_a_reconstruction_tail_is_reconstruct_on_coef_out(shape, with_M):
    from hommx_amd.batch import REGION_FIELDS

    p, d = _case(shape, with_M)
    law, lab = soft_law(p.kind, p.dim), _labels(p)
    kw = dict(max_iter=3, tol=0.0, return_coef=True)
    plain = _secant(p, d, law, **kw)
    r = _secant(p, d, law, reconstruct=True, regions=lab, n_regions=3, **kw)
    _equal(_bits(r), _bits(plain), "the secant outputs")
    want = p.reconstruct(r.coef, d["xi"], d["M"], regions=lab, n_regions=3)
    names = ("mean_strain", "mean_flux", "energy", "max_flux", "argmax_element") + REGION_FIELDS
    _equal([getattr(r.reconstruction, n) for n in names], [getattr(want, n) for n in names], "the reconstruction")
    assert r.reconstruction.region_volume.shape == (NC, 3) and r.criterion is None
    both = _secant(p, d, law, reconstruct=True, criterion=_crit("s[0]"), **kw)  # both tails in one call, no regions
    _equal([getattr(both.reconstruction, n) for n in names[:5]], [getattr(want, n) for n in names[:5]], "the reconstruction beside a criterion")
    _equal(_stats(both.criterion), _stats(p.criterion(r.coef, d["xi"], _crit("s[0]"), d["M"])), "the criterion beside a reconstruction")


def test_the_plan_refuses_what_the_tail_cannot_do():
    p, d = _case("p2", 1)
    law = soft_law(p.kind, p.dim)
    with pytest.raises(ValueError, match="no load term"):
        _secant(p, d, law, _load("p2", 1), True, reconstruct=True)
    with pytest.raises(ValueError, match=r"declares history=2; the law has 0"):
        _secant(p, d, law, criterion=_crit("h[1]", history=2))
    with pytest.raises(ValueError, match=r"reads b\[0\], the nonlinear state"):
        p.criterion(d["coef"], d["xi"], _crit("s[0]*b[0]"), d["M"])
    with pytest.raises(ValueError, match=r"b\[1\] is out of range"):
        _secant(p, d, law, criterion=_crit("b[1]"))
    with pytest.raises(ValueError, match="belong to criterion"):
        _secant(p, d, law, crit_values=True)


# -- b. the state criterion, bit for bit ----------------------------------------------------------------------------------------------------
def _state_crit(p, **kw):
    """Exactly rounded operations only, reading x y p f e s c b h; the last entry of the base among them (b[20] of the Voigt kind)."""
    return _crit(f"{EXACT} + b[{p.n_comp - 1}]*h[0] - min(b[0], c[0])/(1 + abs(h[0] - e[1]))", p=[0.75], fields=1, history=1, **kw)


@pytest.mark.parametrize("shape,with_M", CASES)
def test_b_exact_state_criterion_equals_the_host_twin_bitwise(shape, with_M):
    p, d = _case(shape, with_M)
    law, h = soft_law(p.kind, p.dim, history=[UPDATE]), _history(shape, with_M)
    crit = _state_crit(p)
    assert crit.reads_state and crit.state_indices["b"] == p.n_comp
    r = _secant(p, d, law, history=h, max_iter=2, tol=0.0, return_coef=True, criterion=crit, crit_rows=d["rows"][:, :4], crit_values=True,
                crit_fields=True)
    c = r.criterion
    assert np.array_equal(r.status, np.ones(NC, dtype=np.int64)) and not r.info.any() and not np.array_equal(r.coef, d["coef"])
    host = crit.host_values(c.strain, c.flux, r.coef, d["rows"][:, :3], d["points"], d["rows"][:, 3:4], base=d["coef"], history=h)
    assert c.values.shape == host.shape == (NC, p.n_el) and np.isfinite(host).all()
    assert np.array_equal(c.values, host)
    blind = crit.host_values(c.strain, c.flux, r.coef, d["rows"][:, :3], d["points"], d["rows"][:, 3:4], base=r.coef, history=0.0 * h)
    assert not np.array_equal(host, blind)  # b and h are read, and they are not c and 0
    assert np.array_equal(c.max, host.max(axis=1)) and np.array_equal(c.argmax_element, host.argmax(axis=1))  # the smallest element reaching it
    plain = p.criterion(r.coef, d["xi"], _crit("e[0]"), d["M"], fields=True)  # the state the values were formed on
    assert np.array_equal(c.strain, plain.strain) and np.array_equal(c.flux, plain.flux)


def test_b_an_undeclared_criterion_reads_the_base_on_the_row_of_a_law_with_history():
    p, d = _case("e2", 1)
    law, h = soft_law(p.kind, p.dim, history=[UPDATE]), _history("e2", 1)
    crit = _crit("s[0]/where(b[1] > c[1], 2, 1) + b[0]")  # no history= : the base stands behind the law's history on the row
    c = _secant(p, d, law, history=h, max_iter=2, tol=0.0, return_coef=True, criterion=crit, crit_values=True, crit_fields=True)
    host = crit.host_values(c.criterion.strain, c.criterion.flux, c.coef, d["rows"][:, :3], base=d["coef"], history=h)
    assert np.array_equal(c.criterion.values, host)


# -- c. the slot path -----------------------------------------------------------------------------------------------------------------------
def test_c_slot_path_and_lds_path_on_a_large_cell():
    from hommx_amd import MicroCellPlan

    n = 112  # 8 ndof = 98 KiB: with the 60 KiB of fifteen stack rows above the 150 KiB limit of the reconstruction, with four below it
    p = MicroCellPlan(2, n, "poisson")
    rng = np.random.default_rng(19)
    d = {"coef": np.exp(rng.uniform(-1, 1, (1, p.n_el))), "xi": rng.standard_normal((1, 2)), "M": None,
         "rows": rng.integers(-8, 9, (1, 4)) / 8.0, "points": rng.integers(0, 17, (p.n_el, 2)) / 16.0}
    h = rng.integers(0, 16, (1, p.n_el, 1)) / 8.0
    text = "max(h[0], e[0]**2)*b[0]"
    for _ in range(12):
        text = f"(1 + {text})"
    deep, shallow = _crit(f"c[0]/{text}", history=1), _crit("c[0]/(1 + max(h[0], e[0]**2)*b[0])", history=1)
    law = _law(["c[0]/(1 + max(h[0], e[0]**2))"], history=[UPDATE])  # shallow: the rounds run on the LDS path either way
    assert deep.depth == 16 and shallow.depth <= 5 and law.depth <= 5 and 8 * n * n + 4096 * 15 > 150 * 1024 >= 8 * n * n + 4096 * 4
    want = None
    for name, crit in (("slot", deep), ("lds", shallow)):
        r = _secant(p, d, law, history=h, max_iter=2, tol=0.0, return_coef=True, criterion=crit, crit_values=True, crit_fields=True,
                    reconstruct=True)
        assert not r.info.any() and r.rounds[0] == 2 and r.status[0] == 1
        c = r.criterion
        host = crit.host_values(c.strain, c.flux, r.coef, d["rows"][:, :3], base=d["coef"], history=h)
        assert np.array_equal(c.values, host), name
        want = want or (p.reconstruct(r.coef, d["xi"]), p.criterion(r.coef, d["xi"], _crit("e[0]"), fields=True))
        assert np.array_equal(c.strain, want[1].strain) and np.array_equal(c.flux, want[1].flux), name
        assert np.array_equal(r.reconstruction.mean_flux, want[0].mean_flux) and np.array_equal(r.reconstruction.energy, want[0].energy), name
    p.close()


# -- d. independence ------------------------------------------------------------------------------------------------------------------------
def _staggered(shape):
    """The batch of `shape` with M, its macro strains, loads and histories scaled: the cells stop in different rounds, cell 0 unloads."""
    p, d = _case(shape, 1)
    s = np.array([0.1, 1.0, 3.0])
    return p, dict(d, xi=d["xi"] * s[:, None]), _load(shape, 1) * s[:, None, None], np.array(_history(shape, 1, scale=0.25))


def _damage(p):
    n = p.n_comp
    return _law([f"c[{k}]*{G}" for k in range(n)], matrix=p.kind == "poisson_matrix", history=[KAPPA])


D_KW = dict(max_iter=60, crit_rows=None, crit_values=True, crit_fields=True)


def _d_call(p, d, law, crit, load, h, sel=slice(None), **kw):
    kw = dict(dict(D_KW, crit_rows=d["rows"][sel, :4]), **kw)
    return p.secant(d["coef"][sel], d["xi"][sel], law, d["M"][sel], rows=d["rows"][sel, :3], points=d["points"], history=h[sel], P=load[sel],
                    eigenstrain=True, criterion=crit, **kw)


@pytest.mark.parametrize("shape", ["p2", "e3", "mesh_p2"])
def test_d_the_tail_does_not_depend_on_chunking_position_max_iter_or_outputs(shape, monkeypatch):
    p, d, load, h = _staggered(shape)
    law, crit = _damage(p), _state_crit(p)
    want = _d_call(p, d, law, crit, load, h)
    print(f"{shape}: rounds {want.rounds.tolist()}, max {want.criterion.max.tolist()}")
    assert set(want.status.tolist()) <= {0, 1} and len(set(want.rounds.tolist())) > 1
    bits = _tail_bits(want.criterion)
    _equal(_stats(_d_call(p, d, law, crit, load, h, crit_values=False, crit_fields=False).criterion), bits[:4], "no optional tail output")
    _equal(_stats(_d_call(p, d, law, crit, load, h, crit_fields=False, fields=True, values=True, return_coef=True).criterion), bits[:4],
           "other outputs")
    cut = int(want.rounds.min())
    early = want.rounds <= cut
    assert early.any() and not early.all()
    _equal(_tail_bits(_d_call(p, d, law, crit, load, h, max_iter=cut).criterion), bits, "max_iter", early)
    one = _d_call(p, d, law, crit, load, h, slice(1, 2))
    _equal(_tail_bits(one.criterion), [x[1:2] for x in bits], "a batch of its own")
    order = [2, 0, 1]
    _equal(_tail_bits(_d_call(p, d, law, crit, load, h, order).criterion), [x[order] for x in bits], "batch position")
    monkeypatch.setenv("HOMMX_RECON_MEM_MB", "1")
    _plan.cache_clear()  # the variable is read when a plan is created
    try:
        q = _plan(shape)
        rep = 120  # 360 cells: at least two chunks of 1 MB of correctors and load correctors
        sel = np.tile(np.arange(NC), rep)
        got = _d_call(q, d, law, crit, load, h, sel)
        _equal(_tail_bits(got.criterion), [x[sel] for x in bits], "chunking")
        q.close()
    finally:
        _plan.cache_clear()
        _case.cache_clear()
        _load.cache_clear()


@pytest.mark.parametrize("shape", ["p2", "e3", "mesh_p2"])
def test_d_device_entry_equals_host_entry(shape):
    import torch

    from hommx_amd.batch import CoefStream

    p, d, load, h = _staggered(shape)
    law, crit, lab = _damage(p), _state_crit(p), _labels(p)
    want = _d_call(p, d, law, crit, load, h, return_coef=True)
    recon = p.secant(d["coef"], d["xi"], law, d["M"], rows=d["rows"][:, :3], history=h, max_iter=60, reconstruct=True, regions=lab, n_regions=3)
    dev = torch.device("cuda", p.device)
    keep = []

    def upload(a):
        keep.append(torch.from_numpy(np.array(a)).to(dev))
        return keep[-1].data_ptr()

    def empty(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    out = {"state": empty(NC, 3), "A_eff": empty(NC, p.t, p.t), "coef": empty(*d["coef"].shape), "hist": empty(*h.shape), "crit": empty(NC, 4),
           "values": empty(NC, p.n_el), "strain": empty(NC, p.n_el, p.t), "flux": empty(NC, p.n_el, p.t), "stats": empty(NC, 2 * p.t + 3),
           "rstats": empty(NC, 3, 2 * p.t + 4)}
    ptr = {k: v.data_ptr() for k, v in out.items()}
    common = dict(points_ptr=upload(d["points"]), max_iter=60, history_in_ptr=upload(h), history_out_ptr=ptr["hist"],
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    src, M, xi, rows = CoefStream.sampled(d["coef"]).coef_source(upload), upload(d["M"]), upload(d["xi"]), upload(d["rows"][:, :3])
    p.secant_device(NC, src, M, xi, law, rows, ptr["state"], ptr["A_eff"], coef_ptr=ptr["coef"], P_ptr=upload(load), eigenstrain=True,
                    criterion=crit, crit_rows_ptr=upload(d["rows"][:, :4]), crit_ptr=ptr["crit"], crit_values_ptr=ptr["values"],
                    total_strain_ptr=ptr["strain"], total_flux_ptr=ptr["flux"], **common)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    c = want.criterion
    assert np.array_equal(got["state"], np.stack([want.rounds, want.change, want.status], axis=1).astype(np.float64))
    assert np.array_equal(got["crit"], np.stack([c.max, c.argmax_element.astype(np.float64), c.mean, c.exceed_volume], axis=1))
    for k, a in (("A_eff", want.A_eff), ("coef", want.coef), ("hist", want.history), ("values", c.values), ("strain", c.strain), ("flux", c.flux)):
        assert np.array_equal(got[k], a), k
    p.secant_device(NC, src, M, xi, law, rows, ptr["state"], ptr["A_eff"], stats_ptr=ptr["stats"], n_regions=3,
                    regions_ptr=upload(np.where(lab < 255, lab, 255).astype(np.uint8)), region_stats_ptr=ptr["rstats"], **common)
    torch.cuda.synchronize(dev)
    stats, rstats = out["stats"].cpu().numpy(), out["rstats"].cpu().numpy()
    r, t = recon.reconstruction, p.t
    assert np.array_equal(stats[:, :t], r.mean_strain) and np.array_equal(stats[:, t:2 * t], r.mean_flux) and np.array_equal(stats[:, 2 * t], r.energy)
    assert np.array_equal(rstats[:, :, 0], r.region_volume) and np.array_equal(rstats[:, :, 1 + 2 * t], r.region_energy)


# -- e. the statuses ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_M", [("p2", 1), ("e2", 0), ("mesh_ev3", 1)])
def test_e_status_one_is_evaluated_on_the_last_iterate(shape, with_M):
    p, d = _case(shape, with_M)
    crit = _crit(EXACT, p=[0.75], fields=1, threshold=0.5)
    r = _secant(p, d, soft_law(p.kind, p.dim), max_iter=2, tol=1e-15, return_coef=True, criterion=crit, crit_rows=d["rows"][:, :4],
                crit_values=True, crit_fields=True)
    assert np.array_equal(r.status, np.ones(NC, dtype=np.int64)) and np.array_equal(r.rounds, np.full(NC, 2))
    first = _secant(p, d, soft_law(p.kind, p.dim), max_iter=1, values=True)
    assert np.array_equal(r.coef, first.values.reshape(r.coef.shape))  # c^1: what the law gave in the first round
    want = p.criterion(r.coef, d["xi"], crit, d["M"], rows=d["rows"][:, :4], points=d["points"], values=True, fields=True)
    _equal(_tail_bits(r.criterion), _tail_bits(want), "status 1")


@pytest.mark.parametrize("shape", ["p2", "e2"])
@pytest.mark.parametrize("status", [2, 3])
def test_e_a_cell_of_status_two_or_three_leaves_the_others_alone(shape, status):
    p, d = _case(shape, 1)
    d = dict(d, xi=d["xi"] * np.array([0.1, 1.0, 3.0])[:, None])
    crit = _crit("sqrt(s[0]**2 + s[1]**2)/b[0]")
    if status == 2:
        law = _law([f"{t} + 1e-300/(f[0] - 1)" for t in soft_law(p.kind, p.dim).texts], fields=1)
        good, bad = 0.0, 1.0
    else:
        law = soft_law(p.kind, p.dim, scale="f[0]*", fields=1)
        good, bad = 1.0, -1.0
    rows = np.concatenate([d["rows"][:, :3], np.full((NC, 1), good)], axis=1)
    kw = dict(max_iter=60, return_coef=True, criterion=crit, crit_values=True, crit_fields=True, reconstruct=True)
    want = p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, **kw)
    assert not want.status.any()
    rows[1, 3] = bad
    r = p.secant(d["coef"], d["xi"], law, d["M"], rows=rows, **kw)
    assert r.status.tolist() == [0, status, 0]
    _equal(_tail_bits(r.criterion), _tail_bits(want.criterion), "the other cells", [0, 2])
    for name in ("mean_strain", "mean_flux", "energy", "max_flux", "argmax_element"):
        assert np.array_equal(getattr(r.reconstruction, name)[[0, 2]], getattr(want.reconstruction, name)[[0, 2]]), name
    if status == 2:  # evaluated on the iterate before: the start
        assert np.array_equal(r.coef[1], d["coef"][1])
        on_start = p.criterion(d["coef"][1:2], d["xi"][1:2], _crit("sqrt(s[0]**2 + s[1]**2)/c[0]"), d["M"][1:2], values=True)
        assert np.array_equal(r.criterion.values[1], on_start.values[0])


# -- f. the solver classes ------------------------------------------------------------------------------------------------------------------
def test_f_poisson_hmm_the_damage_driver_is_the_trial_history():
    """Load, unload, reload.  After each converged step one more macro step from its solution u runs the micro iteration AT u, so
    ``history_trial`` belongs to u; ``criterion(driver, u, nonlinear=True)`` runs the same rounds on the same inputs, and the driver is
    made of exactly rounded operations: the values are the trial history, bit for bit, before and after the commit."""
    from hommx_amd import fem, hmm, mesh

    law = hmm.SecantLaw(f"c[0]*{G}", history=[KAPPA], history_names=("kappa",))
    driver = hmm.Criterion(KAPPA, history=1)
    A = lambda x, y: 1.0 + 0.5 * np.sin(2 * np.pi * y[0]) * np.cos(2 * np.pi * y[1]) + 0.1 * x[0]
    h = hmm.PoissonHMM(mesh.create_unit_square(4, 4), A, lambda x: 0.0 * x[0], mesh.create_unit_square(5, 5), 0.05)
    V = h.function_space
    nodes = hmm._box_boundary_nodes(V.mesh)
    u, seen = None, []
    for scale in (1.0, 0.5, 1.5):
        g = fem.Function(V)
        g.x.array[:] = scale * (V.mesh.geometry.x[:, 0] + 0.5 * V.mesh.geometry.x[:, 1] ** 2)
        h.set_boundary_conditions(fem.dirichletbc(g, nodes, V))
        u = h.solve_nonlinear(law, max_iter=60, tol=1e-11, micro_iter=100, micro_tol=1e-13, u0=u).x.array.copy()
        assert not h.secant.status.any() and h.nonlinear_history[-1] <= 1e-11
        h.solve_nonlinear(law, max_iter=1, micro_iter=100, micro_tol=1e-13, u0=u)  # the micro iteration at u itself, from the same history
        trial = h.history_trial.copy()
        before = h.criterion(driver, u, nonlinear=True, values=True)
        assert np.array_equal(before.values, trial[:, :, 0]), scale
        assert np.array_equal(before.secant.rounds, h.secant.rounds) and not before.secant.status.any()
        h.commit_history()
        after = h.criterion(driver, u, nonlinear=True, values=True, cells=np.arange(7, 19), chunk_cells=5)
        assert np.array_equal(after.values, trial[7:19, :, 0]), scale
        seen.append(trial)
    assert np.array_equal(seen[1], seen[0]) and (seen[2] >= seen[0]).all() and (seen[2] > seen[0]).any()
    rec = h.reconstruct(u, nonlinear=True, regions=lambda y: (y[0] > 0.5).astype(int))
    soft = h.criterion(hmm.Criterion("c[0]/b[0]"), u, nonlinear=True, values=True)
    assert rec.region_volume.shape == (32, 2) and np.array_equal(rec.secant.rounds, soft.secant.rounds)
    assert (soft.values <= 1).all() and (soft.values < 1).any() and (soft.values > 0.5).all()


def test_f_linear_elasticity_hmm_with_an_eigenstrain_against_the_plan_level_detour():
    from hommx_amd import fem, hmm, mesh

    A = hmm.TwoPhase(lambda y: y[0] < 0.5, lambda x: hmm.Lame(20.0 + 0.0 * x[0], 10.0 + 0.0 * x[0]),
                     lambda x: hmm.Lame(2.0 + 0.0 * x[0], 1.0 + 0.0 * x[0]))
    h = hmm.LinearElasticityHMM(mesh.create_unit_square(4, 4), A, lambda x: np.array([0.0, -8.0]), mesh.create_unit_square(5, 5), 0.05)
    V = h.function_space
    clamp = fem.locate_dofs_geometrical(V, lambda x: np.isclose(x[0], 0) | np.isclose(x[0], 1) | np.isclose(x[1], 0) | np.isclose(x[1], 1))
    h.set_boundary_conditions(fem.dirichletbc(fem.Function(V), clamp, V))
    E = np.zeros((32, 50, 3))
    E[:, :, :2] = 0.02 + 0.01 * np.arange(32)[:, None, None] / 32
    h.set_eigenstrain(E)
    law = hmm.SecantLaw(lam="c[0]", mu="c[1]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))")
    limits = dict(micro_iter=40, micro_tol=1e-12)
    u = h.solve_nonlinear(law, max_iter=60, tol=1e-8, load=True, **limits).x.array.copy()
    assert h.nonlinear_history[-1] <= 1e-8 and not h.secant.status.any()
    crit = hmm.Criterion.von_mises(2, strength="where(b[1] > 5, 900, 60)")
    r = h.criterion(crit, nonlinear=True, fields=True, values=True)
    assert not r.secant.status.any() and not r.info.any() and r.flux.shape == (32, 50, 3)
    # the detour of the parent commit: the stream to the host, then criterion(coef_out) with the eigenstrain
    cells = np.arange(32)
    stream, kind = h._coef_stream(cells)
    plan, xi = h._ensure_plan(kind), h._macro_strains(cells, u)
    rows, points = h._msh.cell_midpoints()[cells], np.ascontiguousarray(h._cell_mesh.cell_midpoints()[:, :2])
    s = plan.secant(stream, xi, law, rows=rows, points=points, max_iter=40, tol=1e-12, return_coef=True, P=E, eigenstrain=True)
    assert np.array_equal(s.rounds, r.secant.rounds) and np.array_equal(s.A_eff, r.A_eff)
    linear = hmm.Criterion.von_mises(2)
    want = plan.criterion(s.coef, xi, linear, rows=rows, points=points, fields=True, values=True, P=E, eigenstrain=True)
    assert np.array_equal(r.flux, want.flux) and np.array_equal(r.strain, want.strain)
    strength = np.where(plan.expand(stream)[:, :, 1] > 5, 900.0, 60.0)
    assert np.array_equal(r.values, want.values / strength)  # one exactly rounded division by the strength of the BASE phase
    with pytest.raises(RuntimeError, match=r"criterion\(crit, nonlinear=True, fields=True\)"):
        h.reconstruct(nonlinear=True)
