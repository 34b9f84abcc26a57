"""Accuracy at contrast of the load solve on the kept fronts (HOMMX_FLAG_TREE_LOADS) on an MI355X (-m gpu): the load
correctors of the 1e5-contrast case of tests/accuracy_gpu.py -- 3D elasticity 5^3 on the tree, two seeded two-phase cells of contrast 1e5
with M = I + 0.3 N, two loads of order one (accuracy_ref.DERIVED_CASES[6], family 2) -- against the long-double truth of
accuracy_ref.derived_truth, for the unflagged plan (one more elimination with the load rows overridden) and for the flagged plan.

Bound, set before anything was measured: the flagged error is at most 4 x the unflagged one.  The unflagged load rows ride through the
elimination once and come back through the explicit inverses N_i once; the flagged forward pass is a second sweep over the same
explicit inverses (a factor of 2), and the rest is margin.  Each error is the largest over the cells and loads of
max |gpu - T| / max |T| per corrector; both figures are printed.

Measured on an MI355X (DESIGN 4.20 has them as well): unflagged 1.449e-14, flagged 1.449e-14, ratio 1.00."""

import numpy as np
import pytest

import accuracy_ref as R
from hommx_amd import MicroCellPlan

pytestmark = pytest.mark.gpu

CASE, FAMILY = R.DERIVED_CASES[6], 2
RATIO = 4.0


def test_load_correctors_at_contrast_1e5():
    """Both errors are printed (`unflagged` / `flagged`); the bound is their ratio."""
    kernel, ckernel, cs = R.derived_case(CASE)
    family, mf = R.DERIVED_FAMILIES[FAMILY]
    family = family or R.top_family(cs[1])
    assert (kernel, cs[1:4], family, mf) == ("multifrontal", ("elasticity", 3, 5), "tp5", "mild")
    coef, M, g = R.case_inputs(cs, family, mf)
    loads = R.derived_inputs(cs, R.case_inputs(cs, "log2", None)[0][0])["loads"]
    truth = [R.derived_truth(cs[1], g["x"], g["cells"], g["tp"], coef[c], M[c], loads=loads)["load_chi"] for c in range(R.NC)]
    err = {}
    for flagged in (False, True):
        p = MicroCellPlan(cs[2], cs[3], cs[1], tree_loads=flagged)
        assert p.corrector_kernel == ckernel and p.load_kernel == ("multifrontal_subst" if flagged else "multifrontal")
        r = p.loads(coef, loads, M, response=True, return_correctors=True)
        assert not r.info.any()
        per = [[float(np.abs(r.correctors[c][l].astype(R.LD) - T[:, l]).max() / np.abs(T[:, l]).max()) for l in range(loads.shape[0])]
               for c, T in enumerate(truth)]
        err[flagged] = max(max(row) for row in per)
        print(f"load correctors at contrast 1e5, {'flagged' if flagged else 'unflagged'}: per cell and load {per}, worst {err[flagged]:.3e}")
        p.close()
    print(f"ratio flagged / unflagged = {err[True] / err[False]:.2f} (bound {RATIO})")
    assert err[False] > 0.0
    assert err[True] <= RATIO * err[False], err
