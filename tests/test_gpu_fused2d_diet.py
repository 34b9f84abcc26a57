"""The fused 2D kernels compute the bits they computed before the sweep's bookkeeping diet (-m gpu; DESIGN 4.1, "Bookkeeping diet").

The diet takes instructions that do no arithmetic out of accl::Sweep<16> (sweep_acc.h: the pivot check on the scalar unit, no s_nop in front of the
pivots' first FMA, the row-rule selects tied in front of the bulk block), which every fused unit shares: general, unstratified, factor-emitting.  No operation is added,
removed or reordered, so A_H, info and the correctors must be the parent's, bit for bit.  tests/golden/fused2d_diet/fused2d_parent_bits.npz was recorded on an
MI355X with the parent build by `python tests/test_gpu_fused2d_diet.py OUT.npz`, from the same `compute()` the test runs.

Sizes, 8 seeded cells each -- the smallest that reach every sweep variant, the padding and both tile boundaries:
M = None (unstratified units): n = 3, 4, 16 (NB = 16: padded, padded with p0 % 4 == 0, none), 17, 31, 32 (NB = 32: widest padding, one column, none);
M given (general units): n = 3, 17, 32; a batch with a negative and a NaN cell at both block sizes; the factor record's solve (k_poisson2d_fused<32,
true, *> + k_fused2d_subst) at n = 17 with and without M, two cells each.
"""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fused2d_diet", "fused2d_parent_bits.npz")  # a directory of its own: test_gpu_blocked counts golden/*.npz
NC = 8
SIZES_ISO = [3, 4, 16, 17, 31, 32]
SIZES_GEN = [3, 17, 32]
SIZES_BAD = [16, 32]
N_SUBST, NC_SUBST = 17, 2


def _inputs(n, with_M, nc=NC):
    rng = np.random.default_rng(9100 + 10 * n + with_M)
    coef = np.exp(rng.uniform(np.log(0.05), np.log(5.0), size=(nc, 2 * n * n)))
    coef[nc - 1] = np.where(rng.uniform(size=2 * n * n) < 0.5, 1e-4, 1e3)  # one two-valued cell of contrast 1e7
    M = np.eye(2)[None] + 0.3 * rng.standard_normal((nc, 2, 2)) if with_M else None
    return coef, M


def _bad_inputs(n):
    coef, _ = _inputs(n, False)
    coef[1] = -1.0
    coef[3, 5] = np.nan
    return coef


def compute():
    """name -> array: everything the fixture holds, computed by the build under test."""
    from hommx_amd import MicroCellPlan

    out = {}
    for n in sorted(set(SIZES_ISO) | set(SIZES_GEN)):
        p = MicroCellPlan(2, n, "poisson")
        assert p.kernel == "fused2d" and p.corrector_kernel == "fused2d_subst"
        for with_M in (False, True):
            if n not in (SIZES_GEN if with_M else SIZES_ISO):
                continue
            coef, M = _inputs(n, with_M)
            A, info = p.solve(coef, M, return_info=True)
            out[f"A_n{n}_M{int(with_M)}"], out[f"info_n{n}_M{int(with_M)}"] = A, info
        if n in SIZES_BAD:
            A, info = p.solve(_bad_inputs(n), return_info=True)
            out[f"A_bad_n{n}"], out[f"info_bad_n{n}"] = A, info
        if n == N_SUBST:
            for with_M in (False, True):
                coef, M = _inputs(n, with_M, NC_SUBST)
                A, corr, info = p.solve(coef, M, return_info=True, return_correctors=True)
                k = f"n{n}_M{int(with_M)}"
                out["subst_A_" + k], out["subst_corr_" + k], out["subst_info_" + k] = A, corr, info
        p.close()
    return out


@pytest.fixture(scope="module")
def got():
    return compute()


@pytest.fixture(scope="module")
def want():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(got, want):
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("n,with_M", [(n, False) for n in SIZES_ISO] + [(n, True) for n in SIZES_GEN])
def test_tensor_bits(n, with_M, got, want):
    k = f"n{n}_M{int(with_M)}"
    assert not want["info_" + k].any() and np.isfinite(want["A_" + k]).all()
    assert np.array_equal(got["info_" + k], want["info_" + k])
    assert np.array_equal(got["A_" + k], want["A_" + k])


@pytest.mark.parametrize("n", SIZES_BAD)
def test_bad_cells_bits(n, got, want):
    info = want[f"info_bad_n{n}"]
    bad = np.zeros(NC, dtype=bool)
    bad[[1, 3]] = True
    assert np.all(info[bad] > 0) and np.all(info[~bad] == 0)
    assert np.array_equal(got[f"info_bad_n{n}"], info)
    assert np.array_equal(got[f"A_bad_n{n}"][~bad], want[f"A_bad_n{n}"][~bad])
    assert np.array_equal(got[f"A_bad_n{n}"], want[f"A_bad_n{n}"], equal_nan=True)


@pytest.mark.parametrize("with_M", [False, True])
def test_factor_record_solve_bits(with_M, got, want):
    k = f"n{N_SUBST}_M{int(with_M)}"
    assert not want["subst_info_" + k].any() and np.isfinite(want["subst_corr_" + k]).all()
    for what in ("subst_info_", "subst_A_", "subst_corr_"):
        assert np.array_equal(got[what + k], want[what + k]), what + k


if __name__ == "__main__":  # record the fixture with the build that is loaded (the parent's)
    sys.path.insert(0, os.path.dirname(HERE))
    np.savez(sys.argv[1], **compute())
    print("recorded", sys.argv[1], os.path.getsize(sys.argv[1]), "bytes")
