"""The info[] contract on LOCALIZED failures, one small case per route, on an MI355X (-m gpu).

Every batch has 12 cells: 6 good cells interleaved with 6 copies of good cell 0 in which exactly one element is changed -- the first
element, an element at the last (gauge) node, an element at node 0, three seeded random elements (tests/accuracy_gpu.py).  Such a cell
surfaces in ONE late pivot (the last plane, next to the gauge node, a top separator of the tree), not in every lane like the whole-cell
failures of the other suites.  The reference classifies every doctored cell from the eigenvalues of its pinned float64 matrix, and
every cell must be decisive, |lambda_min / lambda_max| > 1e-6:

    indefinite                                        -> info > 0
    SPD although one element is negative or zero      -> info == 0, tensor within the bound of tests/test_gpu_accuracy.py
    one node isolated (all its elements zero)         -> info > 0       (an exactly zero pivot)
    one NaN / +Inf element, one NaN entry of M        -> info > 0

The good cells keep the bits they have in a batch of good cells only.

The same batches through second_sensitivities on one case per load route: the flag, the accuracy of d2A on the cells that stay SPD
(per block, the bound of tests/test_gpu_accuracy_derived.py), the bits of the neighbours.
"""

import numpy as np
import pytest

import accuracy_gpu as G
import accuracy_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cache = {}

    def get(group):
        if group not in cache:
            cache[group] = G.run_pivot_group(group) if group == "default" else G.run_in_child("pivot", group, tmp_path_factory.mktemp(group))
        return cache[group]

    return get


def _spectrum_ratio(kind, x, cells, tp, coef, M):
    """lambda_min / lambda_max of the float64 matrix with node 0 pinned.  (K PSD with the constants as its only kernel <=> this matrix SPD,
    whichever node is pinned: x^T K x = (x - x_0 1)^T K (x - x_0 1).)"""
    a = R.Assembled(kind, x, cells, tp, coef, M, np.float64)
    keep = np.arange(a.bs, a.nd)
    ev = np.linalg.eigvalsh(a.dense()[np.ix_(keep, keep)])
    return ev[0] / ev[-1]


def _check_case(res, key, kind, x, cells, tp, good, M, n_iso, ref_kw):
    cells_p = tp[cells]
    n_nodes = int(tp.max()) + 1
    A0, i0 = res[f"goodA|{key}"], res[f"goodinfo|{key}"]
    assert np.all(i0 == 0)
    batches = G.pivot_batches(kind, cells_p, n_nodes, good, M, n_iso)
    classes = set()
    for name, (coef, MM, where) in batches.items():
        A, info = res[f"A|{key}|{name}"], res[f"info|{key}|{name}"]
        # the good cells: unflagged, and bit for bit what they are in a batch of good cells only
        assert np.all(info[0::2] == 0), (key, name, info)
        assert np.array_equal(A[0::2], A0), (key, name)
        for i in range(6):
            c = 1 + 2 * i
            if name in ("isolated", "nan", "inf", "nanM"):
                assert info[c] > 0, (key, name, i, where[i], info)
                continue
            ratio = _spectrum_ratio(kind, x, cells, tp, coef[c], MM[c])
            assert abs(ratio) > 1e-6, (key, name, i, ratio)  # every generated cell is decisive
            if ratio < 0:
                classes.add("indefinite")
                assert info[c] > 0, (key, name, i, where[i], ratio, info)
            else:
                classes.add("spd")
                assert info[c] == 0, (key, name, i, where[i], ratio, info)
                T = R.truth(kind, x, cells, tp, coef[c], MM[c])
                e = R.float64_errors(kind, x, cells, tp, coef[c], MM[c], T=T, **ref_kw)
                err = R.rel(A[c], T[0])
                print(f"{key} {name} element {where[i]}: ratio {ratio:.1e} e = {err:.2e} bound {e['bound']:.1e}")
                assert err <= e["bound"], (key, name, i, err, e)
    assert classes == {"indefinite", "spd"}, (key, classes)


@pytest.mark.parametrize("group,kernel,kind,dim,n,flags", G.PIVOT_CASES, ids=lambda v: str(v))
def test_localized_failures_structured(results, group, kernel, kind, dim, n, flags):
    good, M, cells_p, nn = G.pivot_inputs_structured(kind, dim, n)
    x, cells, tp = R.structured(dim, n)
    _check_case(results(group), G.skey(kind, dim, n, flags), kind, x, cells, tp, good, M, 1, {"n": n})


@pytest.fixture(scope="module")
def sens2_results():
    return G.run_pivot_sens2_group()


@pytest.mark.parametrize("group,kernel,kind,dim,n,flags", G.PIVOT_SENS2_CASES, ids=lambda v: str(v))
def test_second_derivatives_of_localized_failures(sens2_results, group, kernel, kind, dim, n, flags):
    """second_sensitivities on the same doctored batches, one case per load route: a cell that stays SPD keeps info == 0 and its d2A meets the
    per-block bound of tests/test_gpu_accuracy_derived.py against its OWN long-double truth; an indefinite cell is flagged; every good
    neighbour keeps the bits it has in a batch of good cells only (d2A, dA, A_eff).  Three shared directions, none of them a coefficient."""
    res, key = sens2_results, G.skey(kind, dim, n, flags)
    good, M, cells_p, nn = G.pivot_inputs_structured(kind, dim, n)
    x, cells, tp = R.structured(dim, n)
    dirs = G.pivot_directions(kind, dim, n, good)
    assert np.all(res[f"goodinfo|{key}"] == 0)
    batches = G.pivot_batches(kind, cells_p, nn, good, M)
    classes, failures = set(), []
    for name in G.pivot_sens2_batches(dim):
        coef, MM, where = batches[name]
        d2A, info = res[f"d2A|{key}|{name}"], res[f"info|{key}|{name}"]
        assert np.all(info[0::2] == 0), (key, name, info)
        for q in ("d2A", "dA", "A"):
            assert np.array_equal(res[f"{q}|{key}|{name}"][0::2], res[f"good{q}|{key}"]), (key, name, q)
        for i in range(6):
            c = 1 + 2 * i
            ratio = _spectrum_ratio(kind, x, cells, tp, coef[c], MM[c])
            assert abs(ratio) > 1e-6, (key, name, i, ratio)
            if ratio < 0:
                classes.add("indefinite")
                assert info[c] != 0, (key, name, i, where[i], ratio, info)
                continue
            classes.add("spd")
            assert info[c] == 0, (key, name, i, where[i], ratio, info)
            a = (kind, x, cells, tp, coef[c], MM[c])
            assert R.euler_directions(coef[c], dirs) == []
            T = R.derived_truth(*a, directions=dirs)
            y = R.derived_float64_errors(*a, directions=dirs, T=T, n=n)
            err = R.block_rel(d2A[c], T["d2A"])
            print(f"{key} {name} element {where[i]}: ratio {ratio:.1e} d2A e = {err.max():.2e} float64 {y['e']['d2A'].max():.1e} "
                  f"ratio to the yardstick {(err / (y['bound']['d2A'] / R.FACTOR)).max():.2f}")
            if not np.all(err <= y["bound"]["d2A"]):
                failures.append((key, name, i, err, y["bound"]["d2A"]))
            assert np.array_equal(d2A[c], np.swapaxes(d2A[c], 0, 1)) and np.array_equal(d2A[c], np.swapaxes(d2A[c], 2, 3))
    assert classes == {"indefinite", "spd"}, (key, classes)
    assert not failures, failures


@pytest.mark.parametrize("case", G.PIVOT_MESH, ids=lambda c: c[0])
def test_localized_failures_mesh(results, case):
    kernel, kind, builder, args, route = case
    msh, good, M, cells_p, nn = G.pivot_inputs_mesh(kind, builder, args)
    x, cells, tp = R.mesh_arrays(msh)
    _check_case(results("default"), G.mkey(kind, builder, args, route), kind, x, cells, tp, good, M, 2, {"msh": msh})
