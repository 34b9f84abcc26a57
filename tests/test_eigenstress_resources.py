"""Scratch and spills of EVERY instantiation of k_eigenstress<DIM, KIND> (csrc/loads.hip): the kernel that turns an
eigenstrain into the load P = -material(coef) E, one thread per (cell, load, element).

It holds the t x t material matrix (36 doubles for 3D elasticity), the eigenstrain and one sum, and indexes them with the constants of
unrolled loops only, so it must need no scratch memory and spill nothing -- on the Voigt kind of 3D as on the scalar one of 2D.  It uses
no LDS.  The figures are read from the metadata notes of the gfx950 code object inside the built library (clang-offload-bundler,
llvm-readelf), in the manner of test_expr_program_resources.py: metadata only, no instruction is looked at.
"""

import os
import re
import shutil
import subprocess

import pytest

KERNEL = r"13k_eigenstressILi(\d+)ELi(\d+)E"  # <DIM, KIND>
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
INSTANCES = [(dim, kind) for dim in (2, 3) for kind in range(4)]  # dispatch_dim_kind of kernels.h


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(DIM, KIND): metadata} of every k_eigenstress<DIM, KIND> of the gfx950 code object that holds them."""
    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    tmp = tmp_path_factory.mktemp("eigenstress_co")
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
                key = (int(found.group(1)), int(found.group(2)))
                assert key not in out, name.group(1)
                out[key] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", entry)}
        return out
    pytest.fail("no gfx950 code object of the library holds k_eigenstress<DIM, KIND>")


def test_the_instantiations_are_the_eight_of_the_dispatch(kernels):
    assert set(kernels) == set(INSTANCES)


@pytest.mark.parametrize("dim,kind", INSTANCES)
def test_no_scratch_no_spill_no_lds(kernels, dim, kind):
    md = kernels[(dim, kind)]
    print(f"k_eigenstress<{dim}, {kind}>:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                               "private_segment_fixed_size", "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == 0
