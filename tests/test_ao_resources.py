"""Register and scratch budget of the ambient-occlusion kernels (csrc/ao.hip), read from
the code objects in the built libmcpt.so (no GPU needed): no kernel may use scratch, and
the 1024-thread ones -- one 16-wave workgroup per CU -- must fit 128 VGPRs + AGPRs per
lane.  The names must stay clear of the substrings tests/test_kernel_resources.py and
tests/test_rayquery_resources.py count their kernels by.
"""
import importlib.util
import os
import re

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels


def test_ao_kernels_use_no_scratch_and_fit_their_workgroups(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    kernels = {}
    for co in _code_objects(lib, tmp_path):
        kernels.update(_kernels(co))
    ao = {k: v for k, v in kernels.items() if "ao_walk" in k or "ao_finish" in k}
    walk = {k: v for k, v in ao.items() if "ao_walk" in k}
    # 2 layouts x (lean, counting) x (point form, pixel form), and the finishing kernel
    assert len(walk) == 8 and len(ao) == 9, sorted(ao)
    for name, r in ao.items():
        print(name, r)
        assert "wf_" not in name and "path_kernel" not in name and "rq_trace" not in name, name
        assert r["scratch"] == 0, (name, r)
    big = {k: r for k, r in walk.items() if re.search(r"ao_walkILi1ELi\d+ELi1024E", k)}
    assert len(big) == 4, sorted(walk)
    for name, r in big.items():
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)
    # the lean global-memory kernels are built for the four workgroups per CU their grid launches: 512 / 4
    lean_global = {k: r for k, r in walk.items() if re.search(r"ao_walkILi0ELi\d+ELi256ELb0E", k)}
    assert len(lean_global) == 2, sorted(walk)
    for name, r in lean_global.items():
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)
