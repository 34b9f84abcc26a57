"""Scratch, spill and LDS budget of EVERY instantiation of the two interpreter kernels of csrc/coef_program.hip -- k_expand_program and
k_expand_program_tangent<P> -- now that both read the per-cell row with a stride and load a field where it is read.

A field is not held in a register: at ``X k``, k >= 3, the kernel loads entry k of the cell's row.  So the value kernel must still
need no scratch and hold stack[16][256] doubles of static LDS and nothing else, and every tangent kernel the 16 (1 + P) BLOCK 8 bytes of
test_expr_tangent_resources.py -- whatever instantiations the unit has (a no-field twin would have to meet the same figures).  The
figures are read from the metadata notes of the gfx950 code object inside the built library, in the manner of
test_expr_tangent_resources.py, whose tools this file borrows: metadata only, no instruction is looked at.
"""

import re

from test_expr_tangent_resources import BLOCK, _tool, notes  # noqa: F401  (notes: the fixture)

VALUE_BLOCK, STACK = 256, 16  # BLOCK and PROGRAM_MAX_STACK of coef_program.hip / coef_program.h


def _kernels(notes, pattern):
    """[(name, metadata)] of every kernel of the code object whose name matches."""
    out = []
    for entry in re.split(r"\n  - (?=\.agpr_count:)", notes):
        name = re.search(r"\n\s+\.name:\s+(\S+)", entry)
        if name and re.search(pattern, name.group(1)) and not name.group(1).endswith(".kd"):
            out.append((name.group(1), {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", entry)}))
    return out


def _report(name, md):
    print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                    "group_segment_fixed_size")})


def test_every_value_kernel_has_no_scratch_no_spill_and_its_stack_in_lds(notes):
    found = _kernels(notes, r"16k_expand_program(?!_tangent)")
    assert found, "no metadata of k_expand_program"
    for name, md in found:
        _report(name, md)
        assert md["private_segment_fixed_size"] == 0, name
        assert md["vgpr_spill_count"] == 0, name
        assert md["group_segment_fixed_size"] == STACK * VALUE_BLOCK * 8, name  # stack[16][BLOCK] and nothing else


def test_every_tangent_kernel_has_no_scratch_no_spill_and_its_stack_in_lds(notes):
    found = _kernels(notes, r"k_expand_program_tangentILi\d+E")
    seen = set()
    for name, md in found:
        P = int(re.search(r"k_expand_program_tangentILi(\d+)E", name).group(1))
        seen.add(P)
        _report(name, md)
        assert md["private_segment_fixed_size"] == 0, name
        assert md["vgpr_spill_count"] == 0, name
        assert md["group_segment_fixed_size"] == STACK * (1 + P) * BLOCK[P] * 8, name  # stack[16][1 + P][BLOCK] and nothing else
    assert seen == {1, 2, 4}  # three slots run the kernel of four

