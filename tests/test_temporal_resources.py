"""The temporal-accumulation kernels (csrc/temporal.hip), read from the code objects in the
built libmcpt.so (no GPU needed): one instantiation per mode and per variance on / off, none
with scratch, LDS or a register count that would cost the 16 x 16 workgroups their occupancy.
Their name must stay clear of the substrings the other resource tests count their kernels by.
"""
import importlib.util
import os
import re
import subprocess

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _kernels

OTHERS = ("wf_", "path_kernel", "rq_trace", "ao_walk", "ao_finish", "dl_walk", "dl_finish", "radiance_kernel",
          "radiance_reduce_kernel")


def test_temporal_kernels_are_four_and_use_no_scratch(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                       # no-op when libmcpt.so is up to date
    kernels, lds = {}, {}
    for co in _code_objects(lib, tmp_path):
        kernels.update(_kernels(co))
        txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True,
                             capture_output=True, text=True).stdout
        for block in re.split(r"\n  - (?=\.agpr_count)", txt):
            name = re.search(r"\.name:\s+(\S+)", block)
            if name:
                lds[name.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    tp = {k: v for k, v in kernels.items() if "temporal_reproject" in k}
    # template <bool QE, bool VAR>: 2 modes x variance carried or not
    assert len(tp) == 4, sorted(tp)
    for qe in (0, 1):
        for var in (0, 1):
            assert len([k for k in tp if re.search(rf"temporal_reprojectILb{qe}ELb{var}EE", k)]) == 1, sorted(tp)
    for name, r in tp.items():
        print(name, r, "lds", lds[name])
        assert not any(s in name for s in OTHERS), name
        assert r["scratch"] == 0 and lds[name] == 0, (name, r, lds[name])
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)      # 256-thread workgroups: two or more per SIMD
