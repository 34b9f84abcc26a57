"""Scratch, spill and LDS budget of the forward-mode interpreter k_expand_program_tangent<P>, P = 1, 2, 4 (csrc/coef_program.hip).

The kernel keeps the top of its stack (1 + P doubles), the accumulators of six components (6 (1 + P) doubles) and the cell's x and y in
registers and indexes none of them dynamically, so it must need no scratch and spill nothing; the rest of the stack is static LDS,
16 (1 + P) BLOCK 8 bytes, which must fit the 64 KiB a workgroup may have.  The figures are read from the metadata notes of the gfx950
code object inside the built library (clang-offload-bundler, llvm-readelf), in the manner of test_fused2d_iso_resources.py: metadata
only, no instruction is looked at.
"""

import os
import re
import shutil
import subprocess

import pytest

KERNEL = "k_expand_program_tangentILi{}E"  # <P>
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
BLOCK = {1: 128, 2: 128, 4: 64}  # tangent_block(P) of coef_program.hip


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """The metadata notes of the gfx950 code object that holds the tangent kernels."""
    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    tmp = tmp_path_factory.mktemp("tangent_co")
    data = open(_lib.LIB_PATH, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, data)] + [len(data)]
    for i, (a, b) in enumerate(zip(starts, starts[1:])):
        if KERNEL.format(1).encode() not in data[a:b]:
            continue
        bundle, co = tmp / f"bundle{i}.bin", tmp / f"bundle{i}.co"
        bundle.write_bytes(data[a:b])
        subprocess.run([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={bundle}", f"--output={co}"], check=True,
                       capture_output=True)
        return subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    pytest.fail("no gfx950 code object of the library holds k_expand_program_tangent")


@pytest.mark.parametrize("P", [1, 2, 4])
def test_no_scratch_no_spill_and_lds_within_a_workgroup(notes, P):
    kernel = KERNEL.format(P)
    for entry in re.split(r"\n  - (?=\.agpr_count:)", notes):
        name = re.search(r"\n\s+\.name:\s+(\S+)", entry)
        if name and kernel in name.group(1):
            md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", entry)}
            break
    else:
        pytest.fail(f"no metadata of {kernel}")
    print(f"P = {P}:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                           "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] <= 65536
    assert md["group_segment_fixed_size"] == 16 * (1 + P) * BLOCK[P] * 8  # stack[16][1 + P][BLOCK] and nothing else
