"""Scratch, spill and LDS of EVERY instantiation of k_criterion_state<DIM, KIND, MESH, OUT> (csrc/criterion_state.hip),
pinned the way tests/test_criterion_resources.py pins k_criterion: profiles/criterion_state_resource_usage.txt records the figures.

The kernel keeps the top of its stack, the strain, the flux and the running statistics in registers and indexes none of them
dynamically (x and the 2 t state values are selected by switches on the uniform operand; f[k], y[i], c[k], h[k] and b[k] are loaded
where they are read), so it must need no scratch and spill nothing.  The stack rows below the top and the field are DYNAMIC LDS, sized at launch; the
static LDS is the reduction rows alone: red[8][2] and red_max[8][2] doubles.  The figures are read from the metadata notes of the gfx950
code object inside the built library (clang-offload-bundler, llvm-readelf), in the manner of test_expr_program_resources.py: metadata
only, no instruction is looked at.
"""

import itertools
import os
import re
import shutil
import subprocess

import pytest

KERNEL = r"17k_criterion_stateILi(\d)ELi(\d)ELb([01])ELb([01])EE"  # <DIM, KIND, MESH, OUT>
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
WALK_WAVES = 8  # kWalkWaves of elem_walk.h
REDUCTION_ROWS = 2 * WALK_WAVES * 2 * 8  # red[kWalkWaves][2] and red_max[kWalkWaves][2], doubles
INSTANTIATIONS = list(itertools.product((2, 3), (0, 1, 2, 3), (0, 1), (0, 1)))


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(DIM, KIND, MESH, OUT): metadata} of every k_criterion_state of the gfx950 code object that holds them."""
    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    tmp = tmp_path_factory.mktemp("criterion_state_co")
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
                key = tuple(int(g) for g in found.groups())
                assert key not in out, name.group(1)
                out[key] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", entry)}
        return out
    pytest.fail("no gfx950 code object of the library holds k_criterion_state")


def test_the_instantiations_are_the_eight_pairs_times_geometry_and_out(kernels):
    assert set(kernels) == set(INSTANTIATIONS)


@pytest.mark.parametrize("key", INSTANTIATIONS, ids=lambda k: "dim{}_kind{}_mesh{}_out{}".format(*k))
def test_no_scratch_no_spill_and_static_lds_is_the_reduction_rows(kernels, key):
    md = kernels[key]
    print(key, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                   "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == REDUCTION_ROWS
    assert -(-md["vgpr_count"] // 8) * 8 + md["agpr_count"] <= 256  # 512 threads are two waves per SIMD: at most 256 registers each
