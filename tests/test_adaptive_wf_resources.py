"""The pixel-list generate kernel of the wavefront's adaptive passes in the code
object that ships (no GPU needed): it exists and has no scratch, and the kernel
census tests/test_kernel_resources.py pins is what it was -- the listed passes
add no instantiation of the extend or shade templates.  Register and scratch
figures only, read as that test reads them.
"""
import importlib.util
import os
import re

import pytest

import test_kernel_resources as KR


def test_wf_generate_list_ships_without_scratch_and_the_census_stands(tmp_path):
    if not os.path.exists(os.path.join(KR.LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(KR.ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    kernels = {}
    for co in KR._code_objects(lib, tmp_path):
        kernels.update(KR._kernels(co))
    gen = {k: r for k, r in kernels.items() if "wf_generate_list" in k}
    assert len(gen) == 1, sorted(gen)
    (name, r), = gen.items()
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128, (name, r)
    assert "wf_extend" not in name and "wf_shade_slots" not in name
    # wf_generate itself stays: the QuinEngine and global-layout renders' kernel
    assert len([k for k in kernels if re.search(r"wf_generateE", k)]) == 1, sorted(kernels)
    # the census: six extends, four 512-thread shades at <= 80 VGPRs, one lean packet extend
    assert len([k for k in kernels if "wf_extend" in k]) == 6
    shade = [r for k, r in kernels.items() if re.search(r"wf_shade_slotsILi512E", k)]
    assert len(shade) == 4 and all(r["vgpr"] <= 80 for r in shade), shade
    assert len([k for k in kernels if re.search(r"wf_extend_primaryILi4ELi1024ELb0E", k)]) == 1
    for k, r in kernels.items():
        if "wf_" in k:
            assert r["scratch"] == 0, (k, r)
