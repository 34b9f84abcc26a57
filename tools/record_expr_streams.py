"""Record what the device interpreter of expression coefficients (csrc/coef_program.hip) gives for the programs of
tests/expr_stream_cases.py, as raw float64: the fixture tests/golden/expr_streams/expr_streams_parent.npz of
tests/test_gpu_expr_parent_bits.py.

    python tools/record_expr_streams.py --tree <checkout of the commit to record, its library built> [--out FILE]

Run on an MI355X.  The package is imported from ``--tree`` (default: this tree) and only ``MicroCellPlan.expand`` and
``expand_tangents`` are called.  Per case ``<name>/coef`` is the stream of ``expand`` -- ``expand_tangents`` must return the same
bits, or nothing is written -- ``<name>/dirs`` the tangents where the program has slots, and ``<name>/ops``, ``<name>/consts`` the
program the numbers belong to.  ``rocm`` is the version of the toolchain: its device math library decides the bits of sqrt .. tanh.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rocm_version() -> str:
    import torch

    return str(torch.version.hip)


def record() -> dict:
    import expr_stream_cases as S

    plans, out = {}, {}
    for name, shape, A in S.cases():
        p = plans.setdefault(shape, S.plan(shape))
        stream = S.stream(shape, A)
        coef = p.expand(stream)
        out[f"{name}/ops"], out[f"{name}/consts"] = A.program()
        out[f"{name}/coef"] = coef
        if A.n_params + A.n_fields:
            again, dirs = p.expand_tangents(stream)
            if not np.array_equal(again, coef):
                raise SystemExit(f"{name}: expand_tangents and expand give different streams")
            out[f"{name}/dirs"] = dirs
        if not all(np.all(np.isfinite(out[k])) for k in (f"{name}/coef", f"{name}/dirs") if k in out):
            raise SystemExit(f"{name}: not finite")
        print(name, coef.shape, out.get(f"{name}/dirs", np.zeros(0)).shape, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="the checkout whose hommx_amd (library built) is recorded")
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "expr_streams", "expr_streams_parent.npz"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.tree), os.path.join(HERE, "tests")]
    out = record()
    import hommx_amd

    out["rocm"] = np.array(rocm_version())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {sum(v.size for k, v in out.items() if k.endswith(('coef', 'dirs')))} doubles, "
          f"ROCm {out['rocm']}, package of {os.path.dirname(os.path.abspath(hommx_amd.__file__))}")


if __name__ == "__main__":
    main()
