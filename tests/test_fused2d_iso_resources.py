"""Register, scratch and LDS budget of the unstratified 32-wide fused kernel k_poisson2d_fused<32, false, true>.

Three waves per SIMD need at most 168 registers per lane (512 / 3, allocated in eights) and twelve workgroups per CU at most 13,312 B of LDS each
(160 KiB / 12); a spill to scratch would put memory traffic into the elimination loop.  The figures are read from the metadata notes of the gfx950
code object inside the built library (clang-offload-bundler, llvm-readelf): metadata only, no instruction is looked at.
"""

import os
import re
import shutil
import subprocess

import pytest

KERNEL = "k_poisson2d_fusedILi32ELb0ELb1E"  # <32, false, true>
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def _kernel_metadata(tmp_path):
    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    data = open(_lib.LIB_PATH, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, data)] + [len(data)]
    for i, (a, b) in enumerate(zip(starts, starts[1:])):
        if KERNEL.encode() not in data[a:b]:
            continue
        bundle, co = tmp_path / f"bundle{i}.bin", tmp_path / f"bundle{i}.co"
        bundle.write_bytes(data[a:b])
        subprocess.run([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={bundle}", f"--output={co}"], check=True,
                       capture_output=True)
        notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"\n  - (?=\.agpr_count:)", notes):
            name = re.search(r"\n\s+\.name:\s+(\S+)", entry)
            if name and KERNEL in name.group(1):
                return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", entry)}
    pytest.fail(f"no gfx950 code object of the library holds the metadata of {KERNEL}")


def test_three_waves_per_simd_budget(tmp_path):
    md = _kernel_metadata(tmp_path)
    print({k: md[k] for k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    assert md["vgpr_count"] + md["agpr_count"] <= 168
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] <= 13312
