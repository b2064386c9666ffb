"""Register and scratch budget of the direct-lighting kernels (csrc/direct.hip), read from
the code objects in the built libmcpt.so (no GPU needed): no kernel may use scratch, and
the 1024-thread ones -- one 16-wave workgroup per CU -- must fit 128 VGPRs + AGPRs per
lane, as must the lean global-memory ones (four workgroups of 256 per CU).  The names
must stay clear of the substrings the other resource tests count their kernels by.
"""
import importlib.util
import os
import re

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels

OTHERS = ("wf_", "path_kernel", "rq_trace", "ao_walk", "ao_finish")


def test_direct_kernels_use_no_scratch_and_fit_their_workgroups(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    kernels = {}
    for co in _code_objects(lib, tmp_path):
        kernels.update(_kernels(co))
    dl = {k: v for k, v in kernels.items() if "dl_walk" in k or "dl_finish" in k}
    walk = {k: v for k, v in dl.items() if "dl_walk" in k}
    # 2 layouts x (lean, counting) x (point form, pixel form), and the finishing kernel
    assert len(walk) == 8 and len(dl) == 9, sorted(dl)
    for name, r in dl.items():
        print(name, r)
        assert not any(o in name for o in OTHERS), name
        assert r["scratch"] == 0, (name, r)
    big = {k: r for k, r in walk.items() if re.search(r"dl_walkILi1ELi\d+ELi1024E", k)}
    assert len(big) == 4, sorted(walk)
    for name, r in big.items():
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)
    # the lean global-memory kernels are built for the four workgroups per CU their grid launches: 512 / 4
    lean_global = {k: r for k, r in walk.items() if re.search(r"dl_walkILi0ELi\d+ELi256ELb0E", k)}
    assert len(lean_global) == 2, sorted(walk)
    for name, r in lean_global.items():
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)
