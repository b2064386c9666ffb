"""Budgets of wf_sphere_clip (no GPU needed), read from the shipped code object as
test_kernel_resources.py reads it.  The kernel is the lean LDS extend with one change
in its start-up and runs where that one ran: one 1024-thread workgroup per CU beside
the other stream's 512-thread shade (two <= 80-VGPR waves per SIMD).  So it holds at
most 88 VGPRs + AGPRs and no scratch; its static LDS is the lean LDS extend's (none),
and the launch passes it that kernel's dynamic size (WfRoute::extend_lds, which an
LDS scene's route also reports as mcpt_scene_primary_shade_lds: stack, image, counter
block, direct table).  Its name must stay clear of the patterns the other resource
pins count kernels by, and the library still has exactly six `wf_extend` kernels.
"""
import os
import re
import subprocess

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels

LEAN_LDS_EXTEND = "wf_extendILi1ELi4ELi1024ELb0EE"        # wf_extend<kLayLds, 4, 1024, false>


def _kernels_with_lds(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    out = {}
    for co in _code_objects(lib, tmp_path):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True,
                               capture_output=True, text=True).stdout
        blocks = re.split(r"\n  - (?=\.agpr_count)", notes)
        for name, r in _kernels(co).items():
            block = [x for x in blocks if re.search(r"\.name:\s+%s\s" % re.escape(name), x)][0]
            r["lds"] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
            out[name] = r
    return out


def test_sphere_clip_budgets_and_name(tmp_path):
    ks = _kernels_with_lds(tmp_path)
    mine = {k: v for k, v in ks.items() if "wf_sphere_clip" in k}
    assert len(mine) == 1, sorted(mine)   # lean only: no counting form
    (name, r), = mine.items()
    for pattern in ("wf_extend", "wf_primary_lists", "wf_shade_slots", "wf_primary_shade", "wf_tile_candidates"):
        assert pattern not in name, name
    print(name, r)
    assert r["vgpr"] + r["agpr"] <= 88, r
    assert r["scratch"] == 0, r
    lean = [v for k, v in ks.items() if LEAN_LDS_EXTEND in k]
    assert len(lean) == 1
    assert r["lds"] == lean[0]["lds"] == 0, (r, lean)        # all LDS is the launch's dynamic size
    assert len([k for k in ks if "wf_extend" in k]) == 6, sorted(k for k in ks if "wf_extend" in k)


def test_the_lean_extends_lds_leaves_room_for_the_other_streams_shade(mcpt):
    """the dynamic LDS wf_sphere_clip is launched with is the lean LDS extend's (WfRoute::extend_lds; the GPU
    cases run with it): at scene01's image size the stack, the image, the counter block and the direct
    table, and the other stream's shade still fits beside it"""
    from montecarlopathtracer_amd._capi import lib
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    assert scene.clip_spheres()["mask"] != 0
    image = scene.info()["lds_bytes"]
    dynamic = int(lib().mcpt_scene_primary_shade_lds(scene.handle))      # (an LDS scene's extend_lds)
    assert dynamic == 4 * 1024 * 16 + image + 32 + ((8 * 2 * 4 + 16 + 15) & ~15)
    assert dynamic + 16 * (48 + 4) + 64 <= 160 * 1024
