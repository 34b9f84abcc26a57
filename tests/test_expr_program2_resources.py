"""Scratch, spill, LDS and occupancy class of EVERY instantiation of the second-order interpreter kernel k_expand_program2<P>, P = 1, 2
(csrc/coef_program.hip), in the manner of test_expr_program_resources.py.

The kernel keeps the top of its stack (1 + P + S doubles, S = P (P + 1) / 2 second-order slots), the popped operand, the accumulators
of the values and tangents of six components (6 (1 + P) doubles) and the cell's x and y in registers and indexes none of them
dynamically, so it must need no scratch and spill nothing.  The rest of the stack and the sums of the second-order slots are DYNAMIC
LDS sized by the program's depth and component count at launch, so the code object records no static LDS at all.  The registers must
leave the occupancy class profiles/coef_program_resource_usage.txt records, 2 / 2 waves per SIMD (with the 6 S second-order sums in
registers as well P = 2 took 256 VGPRs and 14 AGPRs: one wave).  The figures are read from the metadata notes of the gfx950 code object inside the built library: metadata only, no instruction is looked at.
"""

import os
import re
import subprocess

import pytest

from test_expr_program_resources import MAGIC, SIMD_REGISTERS, TARGET, _tool

KERNEL = r"17k_expand_program2ILi(\d+)E"  # <P>
WAVES_PER_SIMD = {1: 2, 2: 2}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{P: metadata} of every k_expand_program2<P> of the gfx950 code object that holds them."""
    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    tmp = tmp_path_factory.mktemp("program2_co")
    data = open(_lib.LIB_PATH, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, data)] + [len(data)]
    for i, (a, b) in enumerate(zip(starts, starts[1:])):
        if not re.search(KERNEL.encode(), data[a:b]):
            continue
        bundle, co = tmp / f"bundle{i}.bin", tmp / f"bundle{i}.co"
        bundle.write_bytes(data[a:b])
        subprocess.run([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={bundle}", f"--output={co}"], check=True,
                       capture_output=True)
        notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        out = {}
        for entry in re.split(r"\n  - (?=\.agpr_count:)", notes):
            name = re.search(r"\n\s+\.name:\s+(\S+)", entry)
            found = name and not name.group(1).endswith(".kd") and re.search(KERNEL, name.group(1))
            if found:
                assert int(found.group(1)) not in out, name.group(1)
                out[int(found.group(1))] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", entry)}
        return out
    pytest.fail("no gfx950 code object of the library holds k_expand_program2<P>")


def test_the_instantiations_are_one_and_two_slots(kernels):
    assert set(kernels) == {1, 2}  # three and four slots run the kernel of two once per pair of slots


@pytest.mark.parametrize("P", [1, 2])
def test_no_scratch_no_spill_dynamic_stack_and_occupancy_class(kernels, P):
    md = kernels[P]
    print(f"P = {P}:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                           "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == 0  # stack and second-order sums are dynamic LDS: (depth (1 + P + S) + n_comp S) 64 8 bytes
    registers = -(-md["vgpr_count"] // 8) * 8 + md["agpr_count"]
    by_registers = min(8, SIMD_REGISTERS // registers)
    print(f"P = {P}: {registers} registers allocated: {by_registers} waves per SIMD by registers")
    assert by_registers >= WAVES_PER_SIMD[P]  # at most 256 registers
