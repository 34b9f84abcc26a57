"""Accuracy of everything computed FROM the correctors against extended precision, on an MI355X (-m gpu): reconstruction (strain, flux,
means, energy, max flux, argmax, region rows), coefficient derivatives (dA, grad), stratification derivatives (dA_dM, grad_M), load
responses (P_eff, energy, mean flux, fields, load correctors) and second coefficient derivatives (d2A).

For every returned array of every cell   e = max|gpu - T| / max|T|  <=  32 * max(e_float64, 16 eps),   T = accuracy_ref.derived_truth (long
double), e_float64 the error of the float64 NumPy references of the coarse tests (recon_ref, sens_ref, strat_sens_ref, loads_ref) against
the same truth on the same inputs.  No bound here is computed from a GPU result; tests/test_accuracy_ref_host.py keeps every yardstick
below 1e-11 (correctors 1e-10).  The element the device names as the flux maximum must reach the truth's maximum to within the bound.
d2A takes the rule PER BLOCK (a, b), each block over its own largest entry: the blocks of one cell differ by three orders of magnitude.  The
blocks that vanish by Euler's identity (a direction that is the cell's coefficient; read off the inputs) go over the array's largest entry.
d2A is bitwise symmetric in both index pairs, and it is checked on both load routes of the fused 2D plans: by substitution in process, by
one more elimination of the blocked family in a child process.

Nine cases -- the smallest shapes that reach every (dim, kind, mesh) instantiation of the kernels on every corrector source, asserted
through plan.kernel / plan.corrector_kernel -- with two seeded cells each of log2 without M, log2 and the top-contrast family with
M = I + 0.3 N, log2 with shear 30 and with a squeeze by 16.  Sweeps: one case per corrector path with coef 2^k, M 2^j, loads 2^k; every
output, rescaled by its exact law (accuracy_ref.SCALING_LAWS, decided by the host test), equals the (0, 0) numbers of the device to 16 eps.  Likewise with the directions alone times 2^i: dA by 2^i, d2A by 2^(2i).
"""

import numpy as np
import pytest

import accuracy_gpu as G
import accuracy_ref as R

pytestmark = pytest.mark.gpu

_truth_cache = {}
ARGMAX = {"argmax": ("norm", "max_flux"), "region_argmax": ("region_norm", "region_max_flux"), "load_argmax": ("load_norm", "load_max_flux")}


@pytest.fixture(scope="module")
def results():
    return G.run_derived_group()


def _reference(cs, fi, c, inp):
    """(derived truth, float64 yardsticks and bounds) of one cell, computed once."""
    key = (R.case_id(cs), fi, c)
    if key not in _truth_cache:
        family, mf = R.DERIVED_FAMILIES[fi]
        coef, M, g = R.case_inputs(cs, family or R.top_family(cs[1]), mf)
        args = (cs[1], g["x"], g["cells"], g["tp"], coef[c], None if M is None else M[c])
        T = R.derived_truth(*args, **inp)
        _truth_cache[key] = (T, R.derived_float64_errors(*args, **inp, T=T, **g["kw"]))
    return _truth_cache[key]


def _device(name, v):
    """A device array of one cell in the layout of the truth (correctors: dof first)."""
    return v.T if name == "load_chi" else v


def _family_id(case, fi) -> str:
    family, mf = R.DERIVED_FAMILIES[fi]
    return f"{R.case_id(R.derived_case(case)[2])}-{family or R.top_family(case[2])}-{mf or 'noM'}"


_CELLS = [(c, fi) for c in R.DERIVED_CASES for fi in range(len(R.DERIVED_FAMILIES))]


def _bitwise_symmetric(d2A):
    return np.array_equal(d2A, np.swapaxes(d2A, -1, -2)) and np.array_equal(d2A, np.swapaxes(d2A, -3, -4))


def _check_arrays(got, cs, fi, c, inp, what):
    """Every array of ``got`` that has a yardstick, of cell c, against its own bound -> (number checked, failures).  d2A per block
    (accuracy_ref.block_rel; the Euler blocks, read off the inputs, over the array's largest entry), and bitwise symmetric."""
    T, y = _reference(cs, fi, c, inp)
    checked, failures = 0, []
    for name, bound in y["bound"].items():
        if name not in got:
            continue
        if name == "d2A":
            family, mf = R.DERIVED_FAMILIES[fi]
            coef = R.case_inputs(cs, family or R.top_family(cs[1]), mf)[0][c]
            err = R.block_rel(got[name][c], T[name], R.euler_directions(coef, inp["directions"]))
            if not _bitwise_symmetric(got[name][c]):
                failures.append((what, name, "not bitwise symmetric"))
        else:
            err = R.rel(_device(name, got[name][c]), T[name])
        ratio = np.max(err / (bound / R.FACTOR))
        print(f"{what} {name}: e = {np.max(err):.2e}  float64 {np.max(y['e'][name]):.1e}  bound {np.max(bound):.1e}  ratio {ratio:.2f}")
        checked += 1
        if not np.all(err <= bound):
            failures.append((what, name, err, bound))
    return checked, failures


@pytest.mark.parametrize("case,fi", _CELLS, ids=[_family_id(c, fi) for c, fi in _CELLS])
def test_derived_outputs(results, case, fi):
    """Every returned array of both cells of one case and family against its own bound; info 0; the named elements reach the maximum.

    This test found that the substitution correctors of the fused 2D plans lost a larger multiple of cond(K) eps than a sparse LU
    ([fused2d-poisson-2-16-log2-shear30], second cell, grad_M: ratio 44 of 32 allowed); they now take one refinement step."""
    _, _, cs = R.derived_case(case)
    cid = R.case_id(cs)
    inp = R.derived_inputs(cs, R.case_inputs(cs, "log2", None)[0][0])
    family, mf = R.DERIVED_FAMILIES[fi]
    failures = []
    got = {k.split("|")[3]: v for k, v in results.items() if k.startswith(f"d|{cid}|{fi}|")}
    assert np.all(got["info"] == 0), (cid, fi, got["info"])
    for c in range(R.NC):
        T, y = _reference(cs, fi, c, inp)
        what = f"{cid} {family or R.top_family(cs[1])} M={mf} cell {c}"
        checked, failed = _check_arrays(got, cs, fi, c, inp, what)
        failures += failed
        assert checked == (24 if "load_flux" in got else 17), (what, checked)  # every array the calls return (the frontal mesh route: no load solve, no d2A)
        # the element the device names must reach the maximum of the truth's flux norm to within the bound of that maximum
        for name, (norm, mx) in ARGMAX.items():
            if name not in got:
                continue
            k = np.atleast_1d(got[name][c])
            nrm = np.atleast_2d(T[norm])
            if not np.all(nrm[np.arange(len(k)), k] >= nrm.max(axis=1) * (1 - y["bound"][mx])):
                failures.append((what, name, k, nrm.argmax(axis=1)))
    assert not failures, failures


_FUSED = [c for c in R.DERIVED_CASES if c[0] == "fused2d"]


@pytest.fixture(scope="module")
def blocked_loads(tmp_path_factory):
    return G.run_in_child("derived", "blocked_loads", tmp_path_factory.mktemp("blocked_loads"))


@pytest.mark.parametrize("case", _FUSED, ids=lambda c: R.case_id(R.derived_case(c)[2]))
def test_load_solves_of_the_fused_plans_on_the_blocked_route(blocked_loads, case):
    """HOMMX_FUSED_LOADS=0 (read when a plan is created: one child process): the load solves of the fused 2D plans by one more elimination of
    the blocked family instead of the substitution, route asserted by the runner.  Everything ``loads`` and ``second_sensitivities`` return, every
    family, both cells, to the bounds of test_derived_outputs: a loss on the in-process run alone is the substitution's, one on both is
    of the kernels that form the loads and contract."""
    _, _, cs = R.derived_case(case)
    cid = R.case_id(cs)
    inp = R.derived_inputs(cs, R.case_inputs(cs, "log2", None)[0][0])
    failures = []
    for fi, (family, mf) in enumerate(R.DERIVED_FAMILIES):
        got = {k.split("|")[3]: v for k, v in blocked_loads.items() if k.startswith(f"d|{cid}|{fi}|")}
        assert np.all(got["info"] == 0), (cid, fi, got["info"])
        for c in range(R.NC):
            checked, failed = _check_arrays(got, cs, fi, c, inp, f"blocked loads {cid} {family or R.top_family(cs[1])} M={mf} cell {c}")
            failures += failed
            assert checked == len(R.LOAD_QUANTITIES) + 1, checked  # the load outputs and d2A
    assert not failures, failures


@pytest.mark.parametrize("case", R.DERIVED_SWEEP_CASES, ids=lambda c: R.case_id(R.derived_case(c)[2]))
def test_derived_outputs_under_the_sweeps(results, case):
    """coef 2^k, M 2^j, loads 2^k: a power of two commutes with every rounding, so a route whose arithmetic does not depend on the magnitude
    returns the (0, 0) numbers again after rescaling by the exact law: 16 eps of the largest entry (the precision of the format)."""
    cid = R.case_id(R.derived_case(case)[2])
    pick = lambda k, j: {key.split("|")[4]: v for key, v in results.items() if key.startswith(f"dsw|{cid}|{k}|{j}|")}  # noqa: E731
    base = pick(0, 0)
    failures = []
    for k, j in R.DERIVED_SWEEP_KJ:
        got = pick(k, j)
        assert got.keys() == base.keys()
        assert np.all(got["info"] == 0), (cid, k, j, got["info"])
        for name, v in got.items():
            if name.endswith("argmax") or name == "info":
                assert np.array_equal(v, base[name]), (cid, name, k, j)
                continue
            pk, pj = R.SCALING_LAWS[name]
            d = float(np.abs(v * 2.0 ** -(k * pk + j * pj) - base[name]).max() / np.abs(base[name]).max())
            print(f"sweep {cid} coef 2^{k} M 2^{j} {name}: {d:.2e}")
            if not d <= 16 * R.EPS:
                failures.append((name, k, j, d))
    # directions 2^i alone: dA is linear and d2A bilinear in them (accuracy_ref.DIRECTION_LAWS)
    assert ("d2A" in base) == (case[0] != "mesh_front")
    for i in R.DERIVED_SWEEP_DIR:
        got = {key.split("|")[3]: v for key, v in results.items() if key.startswith(f"ddir|{cid}|{i}|")}
        assert got.keys() == {"dA", "info"} | ({"d2A"} if "d2A" in base else set())
        assert np.all(got["info"] == 0), (cid, i, got["info"])
        for name in got.keys() - {"info"}:
            d = float(np.abs(got[name] * 2.0 ** -(i * R.DIRECTION_LAWS[name]) - base[name]).max() / np.abs(base[name]).max())
            print(f"sweep {cid} directions 2^{i} {name}: {d:.2e}")
            if not d <= 16 * R.EPS:
                failures.append((name, "directions", i, d))
    assert not failures, (cid, failures)
