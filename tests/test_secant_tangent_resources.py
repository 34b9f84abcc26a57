"""Scratch, spill and LDS of EVERY instantiation of k_secant_tangent<DIM, KIND, MESH, P> (csrc/secant_tangent.hip).

The kernel holds the t x P columns of the element tangent that the current sweep forms, the strain and the P tangents of the top of
the stack in registers and indexes none of them dynamically: what depends on the sweep's offset is an address in the element's own
place in the tangent stream, where an entry below the diagonal waits for its pair.  It must need no scratch and spill nothing.  The
stack rows below the top (1 + P doubles per level and thread) and the field are DYNAMIC LDS, sized at launch; the static LDS is the
reduction rows alone, red_max[8][2] doubles for the two maxima of the asymmetry.  P is t for t <= 3 and 2 for t = 6, or 1 (the
fallback for deep programs).  The figures are read from the metadata notes of the gfx950 code object inside the built library, in the
manner of test_secant_resources.py: metadata only, no instruction is looked at.  profiles/secant_tangent_resource_usage.txt holds them.
"""

import itertools
import os
import re
import shutil
import subprocess

import pytest

KERNEL = r"16k_secant_tangentILi(\d)ELi(\d)ELb([01])ELi(\d)EE"  # <DIM, KIND, MESH, P>
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
WALK_WAVES = 8  # kWalkWaves of elem_walk.h
REDUCTION_ROWS = WALK_WAVES * 2 * 8  # red_max[kWalkWaves][2], doubles


def tensor_size(dim, kind):
    """t of kind_sizes (csrc/kernels.h): dim for the Poisson kinds 0, 1; dim (dim + 1) / 2 for the elasticity kinds 2, 3."""
    return dim if kind < 2 else dim * (dim + 1) // 2


def native_slots(t):
    """The widest sweep of secant_tangent_slots: all of t = 2 and t = 3 at once, t = 6 in three sweeps of 2."""
    return t if t <= 3 else 2


INSTANTIATIONS = [(d, k, m, p) for d, k, m in itertools.product((2, 3), (0, 1, 2, 3), (0, 1)) for p in (1, native_slots(tensor_size(d, k)))]


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(DIM, KIND, MESH, P): metadata} of every k_secant_tangent of the gfx950 code object that holds them."""
    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    tmp = tmp_path_factory.mktemp("secant_tangent_co")
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
    pytest.fail("no gfx950 code object of the library holds k_secant_tangent")


def test_the_instantiations_are_the_eight_pairs_times_geometry_and_two_widths(kernels):
    assert set(kernels) == set(INSTANTIATIONS) and len(INSTANTIATIONS) == 32


@pytest.mark.parametrize("key", INSTANTIATIONS, ids=lambda k: "dim{}_kind{}_mesh{}_p{}".format(*k))
def test_no_scratch_no_spill_and_static_lds_is_the_reduction_rows(kernels, key):
    md = kernels[key]
    print(key, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                   "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == REDUCTION_ROWS
    assert -(-md["vgpr_count"] // 8) * 8 + md["agpr_count"] <= 256  # 512 threads are two waves per SIMD: at most 256 registers each


def test_the_stack_rows_fit_the_lds_limit():
    """What secant_tangent_slots decides (csrc/secant_tangent.hip): 512 threads x (1 + P) doubles per level below the top against the
    150 KiB of recon_lds_limit() -- P = 2 to depth 13, P = 3 to depth 10, P = 1 at every depth up to 16."""
    limit = 150 * 1024
    rows = lambda p, depth: 8 * 512 * (1 + p) * (depth - 1)
    assert max(d for d in range(1, 17) if rows(2, d) <= limit) == 13
    assert max(d for d in range(1, 17) if rows(3, d) <= limit) == 10
    assert rows(1, 16) <= limit
