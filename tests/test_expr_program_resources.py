"""Scratch, spill, LDS budget and occupancy class of EVERY instantiation of the interpreter kernel k_expand_program<P>, P = 0 (the
value pass), 1, 2, 4 (csrc/coef_program.hip).

The kernel keeps the top of its stack (1 + P doubles), the accumulators of six components (6 (1 + P) doubles) and the cell's x and y in
registers and indexes none of them dynamically, so it must need no scratch and spill nothing; a field is not held in a register (``X k``,
k >= 3, loads entry k of the cell's row).  The rest of the stack is static LDS, 16 (1 + P) BLOCK 8 bytes and nothing else, which must
fit the 64 KiB a workgroup may have.  The registers must leave the occupancy class profiles/coef_program_resource_usage.txt records,
3 / 2 / 2 / 1 waves per SIMD: a SIMD has 512 registers per lane, allocated in granules of 8.  The figures
are read from the metadata notes of the gfx950 code object inside the built library (clang-offload-bundler, llvm-readelf), in the manner
of test_fused2d_iso_resources.py: metadata only, no instruction is looked at.
"""

import os
import re
import shutil
import subprocess

import pytest

KERNEL = r"16k_expand_programILi(\d+)E"  # <P>
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
STACK = 16  # PROGRAM_MAX_STACK of coef_program.h
BLOCK = {0: 256, 1: 128, 2: 128, 4: 64}  # program_block(P) of coef_program.hip
WAVES_PER_SIMD = {0: 3, 1: 2, 2: 2, 4: 1}
SIMD_REGISTERS = 512


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{P: metadata} of every k_expand_program<P> of the gfx950 code object that holds them."""
    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    tmp = tmp_path_factory.mktemp("program_co")
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
    pytest.fail("no gfx950 code object of the library holds k_expand_program<P>")


def test_the_instantiations_are_the_value_pass_and_one_two_and_four_slots(kernels):
    assert set(kernels) == {0, 1, 2, 4}  # three slots run the kernel of four


@pytest.mark.parametrize("P", [0, 1, 2, 4])
def test_no_scratch_no_spill_stack_in_lds_and_occupancy_class(kernels, P):
    md = kernels[P]
    print(f"P = {P}:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                           "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] <= 65536
    assert md["group_segment_fixed_size"] == STACK * (1 + P) * BLOCK[P] * 8  # stack[16][1 + P][BLOCK] and nothing else
    registers = -(-md["vgpr_count"] // 8) * 8 + md["agpr_count"]
    by_registers = min(8, SIMD_REGISTERS // registers)
    print(f"P = {P}: {registers} registers allocated: {by_registers} waves per SIMD by registers")
    assert by_registers >= WAVES_PER_SIMD[P]  # at most 168 registers for P = 0, 256 for P = 1 and 2
