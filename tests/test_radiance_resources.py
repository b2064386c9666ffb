"""Register and scratch budget of the radiance-query kernels (csrc/render.hip
radiance_kernel), read from the code objects in the built libmcpt.so (no GPU
needed): exactly four instances -- the LDS layout at 1024 threads and the
global-memory layout at 256, each lean and counting -- every one within 128
VGPRs + AGPRs per lane (16 waves per CU), the two lean ones without scratch.
The names must stay clear of the substrings tests/test_kernel_resources.py
counts its kernels by.
"""
import importlib.util
import os
import re

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels


def test_radiance_kernels_fit_their_workgroups(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    kernels = {}
    for co in _code_objects(lib, tmp_path):
        kernels.update(_kernels(co))
    rad = {k: v for k, v in kernels.items() if "radiance_kernel" in k}
    assert len(rad) == 4, sorted(rad)     # 2 layouts x (lean, counting)
    for name, r in rad.items():
        print(name, r)
        assert "wf_" not in name and "path_kernel" not in name, name
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)
    # <IN_LDS, S, BLOCK, COUNT>: one lean and one counting kernel per layout
    for pat in (r"radiance_kernelILb1ELi\d+ELi1024ELb0EE", r"radiance_kernelILb1ELi\d+ELi1024ELb1EE",
                r"radiance_kernelILb0ELi\d+ELi256ELb0EE", r"radiance_kernelILb0ELi\d+ELi256ELb1EE"):
        assert len([k for k in rad if re.search(pat, k)]) == 1, (pat, sorted(rad))
    lean = {k: r for k, r in rad.items() if re.search(r"ELb0EE", k)}
    assert len(lean) == 2, sorted(rad)
    for name, r in lean.items():
        assert r["scratch"] == 0, (name, r)
    # the query's own reduce kernel is there and is none of the four
    red = [k for k in kernels if "radiance_reduce_kernel" in k]
    assert len(red) == 1 and red[0] not in rad
