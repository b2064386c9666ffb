"""Register and scratch budget of the ray-query kernels (csrc/rayquery.hip),
read from the code objects in the built libmcpt.so (no GPU needed): no kernel
may use scratch, and the 1024-thread ones -- one 16-wave workgroup per CU --
must fit 128 VGPRs + AGPRs per lane.  The names must stay clear of the
substrings tests/test_kernel_resources.py counts its kernels by.
"""
import importlib.util
import os
import re

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels


def test_ray_query_kernels_use_no_scratch_and_fit_their_workgroups(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    kernels = {}
    for co in _code_objects(lib, tmp_path):
        kernels.update(_kernels(co))
    rq = {k: v for k, v in kernels.items() if "rq_trace" in k}
    # 2 layouts x (lean, counting) x (closest, any)
    assert len(rq) == 8, sorted(rq)
    for name, r in rq.items():
        print(name, r)
        assert "wf_" not in name and "path_kernel" not in name, name
        assert r["scratch"] == 0, (name, r)
    big = {k: r for k, r in rq.items() if re.search(r"rq_traceILi1ELi\d+ELi1024E", k)}
    assert len(big) == 4, sorted(rq)
    for name, r in big.items():
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)
    # the lean global-memory kernels are built for six waves per SIMD: 512 / 6 -> 80 VGPRs
    lean_global = {k: r for k, r in rq.items() if re.search(r"rq_traceILi0ELi\d+ELi256ELb0E", k)}
    assert len(lean_global) == 2, sorted(rq)
    for name, r in lean_global.items():
        assert r["vgpr"] + r["agpr"] <= 80, (name, r)
