"""Budgets of wf_primary_shade (no GPU needed), read from the shipped code object
as test_kernel_resources.py reads it: the kernel runs one 1024-thread workgroup
per CU beside the other stream's 512-thread shade (two <= 80-VGPR waves per
SIMD), so it must hold what the lean LDS extend holds -- at most 88 VGPRs +
AGPRs, no scratch -- and its LDS is the extend's with its direct table: no
static LDS, and the dynamic size its launch passes (the library reports it from
the function the launch calls, mcpt_scene_primary_shade_lds) at scene01's
image size is at most wf_lds_extend_bytes + kDirectLdsBytes, worked out here
from info()["lds_bytes"]: four 16-B stack entries for each of 1024 lanes, the
image, the 32-B counter block, and the 80-B direct table.
"""
import os
import re
import subprocess

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels


def _primary_shade_kernel(tmp_path):
    """the one kernel that carries the name: its registers, scratch and static LDS"""
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    found = []
    for co in _code_objects(lib, tmp_path):
        ks = {k: v for k, v in _kernels(co).items() if "wf_primary_shade" in k}
        if not ks:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True,
                               capture_output=True, text=True).stdout
        for name, r in ks.items():
            block = [x for x in re.split(r"\n  - (?=\.agpr_count)", notes) if name in x][0]
            r["lds"] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
            found.append((name, r))
    assert len(found) == 1, found         # exactly one kernel carries the name
    return found[0]


def test_primary_shade_budgets(tmp_path):
    name, r = _primary_shade_kernel(tmp_path)
    assert "wf_primary_lists" not in name and "wf_extend" not in name and "wf_tile_candidates" not in name
    assert r["vgpr"] + r["agpr"] <= 88, r
    assert r["scratch"] == 0, r
    assert r["lds"] == 0, r               # all of its LDS is the launch's dynamic size


def test_primary_shade_lds_is_the_lean_extends(mcpt, tmp_path):
    """static + dynamic LDS at scene01's image size <= wf_lds_extend_bytes + kDirectLdsBytes"""
    from montecarlopathtracer_amd._capi import lib
    static = _primary_shade_kernel(tmp_path)[1]["lds"]
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    image = scene.info()["lds_bytes"]
    assert image > 0
    dynamic = int(lib().mcpt_scene_primary_shade_lds(scene.handle))
    assert dynamic > 0
    extend = 4 * 1024 * 16 + image + 32           # wf_lds_extend_bytes: stack, image, counter block
    table = (8 * 2 * 4 + 16 + 15) & ~15           # kDirectLdsBytes: kMaxMissBoxes x kDirectK indices + one 16-B unit
    assert static + dynamic <= extend + table, (static, dynamic, extend, table)
    # and the other stream's shade still fits beside it: its lists' copy, counters and material table
    assert static + dynamic + 16 * (48 + 4) + 64 <= 160 * 1024
    assert int(lib().mcpt_scene_primary_shade_lds(None)) == 0
