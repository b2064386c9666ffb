"""The wavefront radiance queries' kernels in the code object that ships (no GPU
needed; read as test_kernel_resources.py reads it): the generate over ray buffers
and the four forms of the bounce-0 extend that reads its origins from the queue
exist, fit the residency of the extends they stand in for, have no scratch and
no static LDS where the lean LDS extend has none, and their names stay clear of
the patterns the other resource tests count the pipeline's kernels by -- whose
census stands unchanged.
"""
import importlib.util
import os
import re
import subprocess

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels

# the substrings other tests count or select wavefront kernels by
CENSUS = ("wf_extend", "wf_generate_list", "wf_generateE", "wf_shade_slots", "wf_primary_lists", "wf_primary_shade",
          "wf_tile_candidates", "wf_sphere_clip")
FORMS = {"lds_lean": r"wf_ray_extend0ILi1ELi4ELi1024ELb0EE", "lds_count": r"wf_ray_extend0ILi1ELi4ELi1024ELb1EE",
         "global_lean": r"wf_ray_extend0ILi0ELi\d+ELi256ELb0EE", "global_count": r"wf_ray_extend0ILi0ELi\d+ELi256ELb1EE"}


def _static_lds(co):
    """kernel name -> .group_segment_fixed_size of the code object's notes"""
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                         text=True).stdout
    out = {}
    for block in re.split(r"\n  - (?=\.agpr_count)", txt):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    ks = {}
    for co in _code_objects(lib, tmp_path_factory.mktemp("co")):
        lds = _static_lds(co)
        for name, r in _kernels(co).items():
            ks[name] = dict(r, lds=lds[name])
    return ks


def test_the_ray_generate_and_the_four_ray_extends_exist(kernels):
    gen = [k for k in kernels if "wf_ray_generate" in k]
    ext = [k for k in kernels if "wf_ray_extend0" in k]
    assert len(gen) == 1, gen
    assert len(ext) == 4, sorted(ext)
    for key, pat in FORMS.items():
        assert len([k for k in ext if re.search(pat, k)]) == 1, (key, sorted(ext))


def test_they_fit_the_extends_they_stand_in_for(kernels):
    new = {k: r for k, r in kernels.items() if "wf_ray_generate" in k or "wf_ray_extend0" in k}
    assert len(new) == 5
    for name, r in new.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)

    def one(key):
        return [r for k, r in new.items() if re.search(FORMS[key], k)][0]

    # beside two <= 80-VGPR shade waves per SIMD, all of its LDS dynamic (WfRoute::extend_lds)
    assert one("lds_lean")["vgpr"] + one("lds_lean")["agpr"] <= 88, one("lds_lean")
    assert one("lds_lean")["lds"] == 0, one("lds_lean")
    # six workgroups per CU
    assert one("global_lean")["vgpr"] + one("global_lean")["agpr"] <= 80, one("global_lean")


def test_no_new_name_contains_a_census_pattern(kernels):
    for name in kernels:
        if "wf_ray_" in name:
            for pat in CENSUS:
                assert pat not in name, (name, pat)


def test_the_census_of_the_pipeline_stands(kernels):
    assert len([k for k in kernels if "wf_extend" in k]) == 6
    shade = [r for k, r in kernels.items() if re.search(r"wf_shade_slotsILi512E", k)]
    assert len(shade) == 4 and all(r["vgpr"] <= 80 for r in shade), shade
    assert len([k for k in kernels if "wf_generate_list" in k]) == 1
    assert len([k for k in kernels if "wf_generateE" in k]) == 1
    for name, r in kernels.items():
        if "wf_" in name:
            assert r["scratch"] == 0, (name, r)
