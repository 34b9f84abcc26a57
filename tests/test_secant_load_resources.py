"""Scratch, spill and LDS of EVERY instantiation of the two kernels of a law beside a load:
k_secant_load<DIM, KIND, MESH, OUT, HIST> (csrc/secant_load.hip) and k_secant_tangent_load<DIM, KIND, MESH, P, HIST>
(csrc/secant_tangent_load.hip).

Each shares its body with its siblings without a load (secant_round.h, secant_tangent_cell.h) and adds one vector load per dof in the
pass that forms X, and per element the t entries of P or E: nothing is held beside them.  They are held to what the siblings are held
to (test_secant_resources.py, test_secant_tangent_resources.py, test_secant_history_resources.py): no scratch, no spill, static LDS
equal to the reduction rows alone -- red[8][t] and red_max[8][3] doubles for the round, red_max[8][2] for the tangent --, at most 256
registers.  The figures are read from the metadata notes of the gfx950 code object inside the built library: metadata only, no
instruction is looked at.  profiles/secant_load_resource_usage.txt holds them.
"""

import itertools
import re
import subprocess

import pytest

from test_secant_history_resources import MAGIC, TARGET, _tool, native_slots, static_lds, tensor_size

ROUND = r"13k_secant_loadILi(\d)ELi(\d)ELb([01])ELb([01])ELb([01])EE"  # <DIM, KIND, MESH, OUT, HIST>
TANGENT = r"21k_secant_tangent_loadILi(\d)ELi(\d)ELb([01])ELi(\d)ELb([01])EE"  # <DIM, KIND, MESH, P, HIST>

ROUNDS = list(itertools.product((2, 3), (0, 1, 2, 3), (0, 1), (0, 1), (0, 1)))
TANGENTS = [(d, k, m, p, h) for d, k, m in itertools.product((2, 3), (0, 1, 2, 3), (0, 1)) for p in (1, native_slots(tensor_size(d, k)))
            for h in (0, 1)]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{"round" / "tangent": {template arguments: metadata}} of every instantiation in the gfx950 code objects of the library."""
    import os

    from hommx_amd import _lib

    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf of the ROCm LLVM not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    tmp = tmp_path_factory.mktemp("secant_load_co")
    data = open(_lib.LIB_PATH, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, data)] + [len(data)]
    out = {"round": {}, "tangent": {}}
    for i, (a, b) in enumerate(zip(starts, starts[1:])):
        if not re.search((ROUND + "|" + TANGENT).encode(), data[a:b]):
            continue
        bundle, co = tmp / f"bundle{i}.bin", tmp / f"bundle{i}.co"
        bundle.write_bytes(data[a:b])
        subprocess.run([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={bundle}", f"--output={co}"], check=True,
                       capture_output=True)
        notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"\n  - (?=\.agpr_count:)", notes):
            name = re.search(r"\n\s+\.name:\s+(\S+)", entry)
            if not name or name.group(1).endswith(".kd"):
                continue
            for which, pattern in (("round", ROUND), ("tangent", TANGENT)):
                found = re.search(pattern, name.group(1))
                if found:
                    key = tuple(int(g) for g in found.groups())
                    assert key not in out[which], name.group(1)
                    out[which][key] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*(?:\n|$)", entry)}
    if not out["round"] and not out["tangent"]:
        pytest.fail("no gfx950 code object of the library holds k_secant_load or k_secant_tangent_load")
    return out


def test_the_instantiations_are_those_of_the_siblings_with_and_without_history(kernels):
    assert set(kernels["round"]) == set(ROUNDS)
    assert set(kernels["tangent"]) == set(TANGENTS)


@pytest.mark.parametrize("which,key", [("round", k) for k in ROUNDS] + [("tangent", k) for k in TANGENTS],
                         ids=lambda v: v if isinstance(v, str) else "dim{}_kind{}_mesh{}_{}_hist{}".format(*v))
def test_no_scratch_no_spill_and_static_lds_is_the_reduction_rows(kernels, which, key):
    md = kernels[which][key]
    print(which, key, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                          "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == static_lds(which, key[0], key[1])
    assert -(-md["vgpr_count"] // 8) * 8 + md["agpr_count"] <= 256  # 512 threads are two waves per SIMD: at most 256 registers each
