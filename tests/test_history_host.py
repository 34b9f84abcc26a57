"""History variables of a ``SecantLaw`` on the CPU: the grammar of ``h[k]`` and ``history=``, the row and the STORE order
of ``program``, the limits for components and updates together, a law without history compiling to what it compiled to, the twins
``host_values(history=)`` / ``host_history`` against the formula, ``host_tangent(history=)`` against central differences on the loading
and on the unloading branch, and the load / unload / reload path of one cell on tests/history_ref.py.  No GPU.
"""

import numpy as np
import pytest

import history_ref as H
import recon_ref as R
from hommx_amd.expr import MAX_HISTORY, OP_CONST, OP_MAX, OP_STORE, OP_X, Criterion, SecantLaw

EQ = "sqrt(e[0]**2 + e[1]**2)"
DAMAGE = f"c[0]*(1 - 0.5*(1 - exp(-max(h[0], {EQ})/0.7)))"
KAPPA = f"max(h[0], {EQ})"


def damage_law():
    return SecantLaw(DAMAGE, history=[KAPPA], history_names=("kappa",))


# -- the grammar ---------------------------------------------------------------------------------------------------------------------------
def test_h_without_history_is_refused_naming_the_node():
    with pytest.raises(ValueError, match=r"h\[k\] needs the updates of the history variables \(history=\[\.\.\.\]\): Subscript 'h\[0\]'"):
        SecantLaw("c[0]*h[0]")
    with pytest.raises(ValueError, match=r"Subscript 'h\[1\]'"):
        SecantLaw(lam="c[0]", mu="c[1] + h[1]")
    with pytest.raises(ValueError, match=r"h\[k\] needs"):  # a criterion has no history: out of scope
        Criterion("s[0] + h[0]")


def test_an_index_at_or_above_n_history_is_refused():
    with pytest.raises(ValueError, match=r"below the number of history variables \(1\): Subscript 'h\[1\]'"):
        SecantLaw("c[0]*h[1]", history=["h[0]"])
    with pytest.raises(ValueError, match=r"below the number of history variables \(2\): Subscript 'h\[2\]'"):
        SecantLaw("c[0]", history=["h[0]", "h[2]"])
    with pytest.raises(ValueError, match=r"Subscript 'h\[-1\]'|h\[-1\]"):
        SecantLaw("c[0]*h[-1]", history=["h[0]"])


def test_the_count_the_names_and_the_initial_values():
    assert MAX_HISTORY == 4
    for bad in ([], ["h[0]"] * 5):
        with pytest.raises(ValueError, match="history has 1 .. 4 update texts"):
            SecantLaw("c[0]", history=bad)
    with pytest.raises(ValueError, match="2 history_names for 1 history variables"):
        SecantLaw("c[0]", history=["h[0]"], history_names=("a", "b"))
    with pytest.raises(ValueError, match="history_names without history"):
        SecantLaw("c[0]", history_names=("a",))
    with pytest.raises(ValueError, match="history_initial"):
        SecantLaw("c[0]", history=["h[0]", "h[1]"], history_initial=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="history_initial"):
        SecantLaw("c[0]", history=["h[0]"], history_initial=float("nan"))
    law = SecantLaw("c[0]", history=["h[0]", "h[1] + 1", "h[2]", "h[3]"], history_initial=0.25)
    assert law.n_history == 4 and law.history_names == ("h0", "h1", "h2", "h3") and np.array_equal(law.history_initial, [0.25] * 4)
    assert np.array_equal(SecantLaw("c[0]", history=["h[0]", "h[1]"], history_initial=[1.0, 2.0]).history_initial, [1.0, 2.0])
    plain = SecantLaw("c[0]")
    assert plain.n_history == 0 and plain.history_names == () and plain.history_initial.shape == (0,)
    assert damage_law().history_names == ("kappa",) and damage_law().n_history == 1


# -- the program ---------------------------------------------------------------------------------------------------------------------------
def test_the_row_indices_and_the_store_order():
    law = SecantLaw(lam="c[0] + f[1]*e[2] + h[1]", mu="c[1]*h[0] + x[1]", fields=2, history=["max(h[0], e[0])", "h[1] + c[1]*y[0]"])
    ops, consts = law.program(3, 2)  # row: [midpoint 3 | fields 2 | e 3 | s 3 | c 2 | h 2]
    assert [int(k) for op, k in ops if op == OP_X] == [11, 4, 7, 14, 12, 13, 1, 13, 5, 14, 12]
    stores = [i for i, (op, k) in enumerate(ops) if op == OP_STORE]
    assert [int(ops[i][1]) for i in stores] == [0, 1, 2, 3] and stores[-1] == len(ops) - 1  # the components first, then the updates
    assert law.n_law_ops == stores[1] + 1  # the tangent pass runs the program truncated behind the last component's STORE
    assert law.state_indices == {"e": 3, "s": 0, "c": 2, "h": 2} and law.explicit
    assert ops.dtype == np.uint8 and ops[:, 0].max() <= OP_STORE  # no opcode is added
    ops6, _ = law.program(6, 2)
    assert [int(k) for op, k in ops6 if op == OP_X] == [17, 4, 7, 20, 18, 19, 1, 19, 5, 20, 18]
    with pytest.raises(ValueError, match="it has 2 components; the plan's coefficient has n_comp = 1"):
        law.program(2, 1)


def test_explicit_counts_the_updates():
    assert not SecantLaw("c[0]", history=["max(h[0], abs(s[0]))"]).explicit
    assert SecantLaw("c[0]/(1 + h[0])", history=["max(h[0], abs(e[0]))"]).explicit
    with pytest.raises(ValueError, match=r"s\[1\]"):
        SecantLaw("c[0]", history=["h[0] + s[1]"]).host_tangent(np.zeros((1, 2, 2)), np.ones((1, 2)), np.ones((1, 2)), np.zeros((1, 3)),
                                                               history=np.zeros((1, 2, 1)))


def test_the_limits_hold_for_components_and_updates_together():
    terms = lambda n, name="e[0]": " + ".join([name] * n)  # n reads and n - 1 sums: 2 n - 1 instructions
    assert len(SecantLaw(terms(32), history=[terms(32)]).program(2, 1)[0]) == 128  # 63 + 1 + 63 + 1
    with pytest.raises(ValueError, match="too long: 130 instructions, at most 128"):
        SecantLaw(terms(32), history=[terms(33)])
    many = lambda a, b: "e[0] + " + " + ".join(f"{k}.5" for k in range(a, b))  # a varying left operand: nothing folds
    assert len(SecantLaw(many(0, 16), history=[many(16, 32)]).program(2, 1)[1]) == 32
    with pytest.raises(ValueError, match="too many constants: 33"):
        SecantLaw(many(0, 16), history=[many(16, 33)])
    deep = lambda n: "e[0] + (" * (n - 1) + "e[0]" + ")" * (n - 1)
    assert SecantLaw("c[0]", history=[deep(16)]).depth == 16
    with pytest.raises(ValueError, match="too deep: stack depth 17, at most 16"):
        SecantLaw("c[0]", history=[deep(17)])


def test_a_law_without_history_compiles_to_what_it_compiled_to():
    """The ops and consts of two laws as the version before the history variables wrote them, literally."""
    ops, consts = SecantLaw("c[0]*(0.5 + 0.5/(1 + e[0]**2 + e[1]**2))").program(2, 1)
    assert ops.tolist() == [[1, 7], [0, 0], [0, 0], [0, 1], [1, 3], [26, 0], [5, 0], [3, 0], [1, 4], [26, 0], [5, 0], [3, 0], [6, 0], [3, 0],
                            [5, 0], [27, 0]]
    assert consts.tolist() == [0.5, 1.0]
    law = SecantLaw(lam="c[0]", mu="c[1]*p[0]/(1 + f[0]*s[2]**2) + y[1]", p=[0.25], fields=1)
    ops, consts = law.program(3, 2)
    assert ops.tolist() == [[1, 10], [27, 0], [1, 11], [0, 0], [5, 0], [0, 1], [1, 3], [1, 9], [26, 0], [5, 0], [5, 0], [3, 0], [6, 0], [2, 1],
                            [3, 0], [27, 1]]
    assert consts.tolist() == [0.25, 1.0]
    assert law.state_indices == {"e": 0, "s": 3, "c": 2} and law.n_law_ops == len(ops)


def test_the_damage_law_reads_h_through_max_and_stores_kappa_last():
    ops, consts = damage_law().program(2, 1)
    assert [int(k) for op, k in ops if op == OP_X] == [7, 8, 3, 4, 8, 3, 4]  # c, h, e, e | h, e, e
    assert (ops[:, 0] == OP_MAX).sum() == 2 and ops[-1].tolist() == [OP_STORE, 1]
    assert [float(consts[k]) for op, k in ops if op == OP_CONST] == [1.0, 0.5, 1.0, 0.7]


# -- the twins -----------------------------------------------------------------------------------------------------------------------------
def _dyadic(rng, *shape):
    return rng.integers(-16, 17, shape) / 8.0


def test_host_values_and_host_history_are_the_formula():
    rng = np.random.default_rng(5)
    N, n_el = 3, 7
    e, s = _dyadic(rng, N, n_el, 2), _dyadic(rng, N, n_el, 2)
    c = 1.0 + np.abs(_dyadic(rng, N, n_el))
    x, y, f = _dyadic(rng, N, 3), _dyadic(rng, n_el, 2), _dyadic(rng, N, 1)
    h = _dyadic(rng, N, n_el, 2)
    law = SecantLaw("c[0]*(1 + h[0]) + f[0]*e[1] - h[1]*s[0] + x[2]", fields=1,
                    history=["max(h[0], abs(e[0]) + y[1])", "h[1] + 0.5*(s[1] - h[0])*c[0]"])
    v = law.host_values(e, s, c, x, y, f, history=h)
    g = law.host_history(e, s, c, x, y, f, history=h)
    assert v.shape == (N, n_el, 1) and g.shape == (N, n_el, 2)
    assert np.array_equal(v[:, :, 0], c * (1 + h[:, :, 0]) + f * e[:, :, 1] - h[:, :, 1] * s[:, :, 0] + x[:, 2, None])
    assert np.array_equal(g[:, :, 0], np.maximum(h[:, :, 0], np.abs(e[:, :, 0]) + y[None, :, 1]))
    assert np.array_equal(g[:, :, 1], h[:, :, 1] + 0.5 * (s[:, :, 1] - h[:, :, 0]) * c)
    one = SecantLaw("c[0]*h[0]", history=["h[0] + 1"])
    assert np.array_equal(one.host_history(e, s, c, x, history=h[:, :, 0])[:, :, 0], h[:, :, 0] + 1)  # [N, n_el] for one variable
    with pytest.raises(ValueError, match=r"pass history\[N, n_el, 2\]"):
        law.host_values(e, s, c, x, y, f)
    with pytest.raises(ValueError, match=r"pass history\[N, n_el, 2\]"):
        law.host_history(e, s, c, x, y, f, history=h[:, :, :1])
    with pytest.raises(ValueError, match="no history variables"):
        SecantLaw("c[0]").host_values(e, s, c, x, history=h)
    with pytest.raises(ValueError, match="no history variables"):
        SecantLaw("c[0]").host_history(e, s, c, x)


@pytest.mark.parametrize("branch", ["loading", "unloading"])
def test_host_tangent_with_history_equals_central_differences_of_host_values(branch):
    """T = d(L(e, h) e)/de at frozen h: every element loads (eq > h + 1e-3: max takes eq, the law softens with e) or every element
    unloads (eq < h - 1e-3: max takes h, T is the secant coefficient).  No element sits on the kink, so the differences (h = 1e-6) hold
    to 1e-8 of the largest entry, the bound of test_secant_tangent_host.py."""
    rng = np.random.default_rng(11)
    N, n_el = 2, 9
    e = rng.standard_normal((N, n_el, 2))
    eq = np.sqrt((e**2).sum(axis=2))
    hist = (eq * 0.5 if branch == "loading" else eq * 1.5 + 0.01)[:, :, None]
    assert (np.abs(eq - hist[:, :, 0]) > 1e-3).all()
    base = 1.0 + rng.random((N, n_el))
    law, x = damage_law(), np.zeros((N, 3))
    flux = lambda ee: law.host_values(ee, np.zeros_like(ee), base, x, history=hist) * ee
    cur = law.host_values(e, np.zeros_like(e), base, x, history=hist)
    T, asym = law.host_tangent(e, cur, base, x, history=hist)
    step, F = 1e-6, np.zeros_like(T)
    for n in range(2):
        d = np.zeros(2)
        d[n] = step
        F[..., n] = (flux(e + d) - flux(e - d)) / (2 * step)
    err = np.abs(T - F).max() / np.abs(T).max()
    print(branch, f"|T - FD| = {err:.2e}", "asymmetry", asym)
    assert err <= 1e-8
    secant = cur[:, :, :, None] * np.eye(2)
    if branch == "unloading":
        assert np.array_equal(T, secant) and np.all(asym == 0.0)
    else:
        assert np.abs(T - secant).max() > 1e-2
    with pytest.raises(ValueError, match=r"pass history\[N, n_el, 1\]"):
        law.host_tangent(e, cur, base, x)


# -- the load / unload / reload path of one cell ---------------------------------------------------------------------------------------
N_MICRO, XI, TOL = 8, np.array([1.0, 0.3]), 1e-12


@pytest.fixture(scope="module")
def path():
    """2D Poisson, n = 8: base 10 on 30 % of the elements drawn by default_rng(1), 1 elsewhere; the damage law; load xi from h = 0,
    unload to xi / 2 and reload to 1.5 xi with the committed history, and a virgin cell at xi / 2."""
    n_el = 2 * N_MICRO**2
    base = np.where(np.random.default_rng(1).random(n_el) < 0.3, 10.0, 1.0)
    law, solve = damage_law(), H.solver("poisson", 2, N_MICRO)
    run = lambda xi, h: H.iterate(solve, law, base, xi, h, max_iter=100, tol=TOL)
    load = run(XI, np.zeros((n_el, 1)))
    unload = run(0.5 * XI, load["history"])
    reload_ = run(1.5 * XI, unload["history"])
    virgin = run(0.5 * XI, np.zeros((n_el, 1)))
    return {"base": base, "law": law, "load": load, "unload": unload, "reload": reload_, "virgin": virgin}


def test_loading_converges_and_every_element_remembers_its_largest_strain(path):
    r = path["load"]
    print("loading rounds", r["rounds"], "change", r["change"])
    assert r["status"] == 0 and r["rounds"] == 19
    eq = np.sqrt((r["s"]**2).sum(axis=1))
    assert np.array_equal(r["history"][:, 0], eq) and (eq > 0).all()


def test_unloading_stops_in_two_rounds_on_the_damaged_coefficient_and_leaves_the_history(path):
    r, before = path["unload"], path["load"]["history"]
    assert r["status"] == 0 and r["rounds"] == 2
    assert np.array_equal(r["history"], before)  # not a bit
    law, base = path["law"], path["base"]
    zero = np.zeros((1, len(base), 2))
    damaged = law.host_values(zero, zero, base[None], np.zeros((1, 3)), history=before[None])[0, :, 0]
    linear = R.structured("poisson", 2, N_MICRO, damaged, None, 0.5 * XI)["A"]
    dev = np.abs(r["A"] - linear).max() / np.abs(linear).max()
    print("unloading: A against the linear solve on the damaged coefficient", dev)
    assert dev <= 1e-12


def test_reloading_grows_every_history_and_the_response_is_path_dependent(path):
    r = path["reload"]
    print("reloading rounds", r["rounds"])
    assert r["status"] == 0 and r["rounds"] == 20
    assert (r["history"] > path["unload"]["history"]).all()
    apart = np.abs(path["virgin"]["A"] - path["unload"]["A"]).max()
    print("virgin against unloaded at xi / 2:", apart)
    assert apart > 0.1
    assert path["virgin"]["status"] == 0 and (path["virgin"]["history"] < path["load"]["history"]).all()
