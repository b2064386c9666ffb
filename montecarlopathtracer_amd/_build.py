"""Build libmcpt.so (HIP for gfx950 + C++ host) in-tree with hipcc.

Output: montecarlopathtracer_amd/lib/libmcpt.so.  Every translation unit is
compiled with -ffp-contract=off and without fast-math: the kernel's float
arithmetic must round exactly as the specification.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, os.environ.get("MCPT_LIB_NAME", "libmcpt.so"))
SOURCES = ["host_model.cpp", "kd_cache.cpp", "capi.cpp", "scene_image.cpp", "plan.cpp", "render_host.cpp", "queries.cpp",
           "render.hip", "wavefront.hip", "wavefront_primary.hip", "wavefront_primary_shade.hip",
           "wavefront_sphere.hip", "wavefront_rays.hip", "aov.hip", "denoise.hip", "variance.hip", "denoise_var.hip", "adaptive.hip", "rayquery.hip", "ao.hip",
           "direct.hip", "temporal.hip"]
# per-source code generation (wavefront_primary.hip: the bounce-0 packet extend's
# wave-uniform control flow as scalar branches; render.hip: GVN hoisting,
# megakernel +1.4%, no effect on the wavefront kernels, and the global-memory
# variants' capped descent unrolled (C4 megakernel +2.1%); the wavefront kernels:
# wave priority raised around their vector-memory loads, C2 +0.4%, and
# if-diamonds of up to 8 instructions folded into selects and the capped
# descent unrolled -- only the global-memory extends change, C4 +0.9% and +3.0%)
_WF_FLAGS = ["-mllvm", "-amdgpu-set-wave-priority=1", "-mllvm", "-two-entry-phi-node-folding-threshold=8",
             "-mllvm", "-unroll-threshold=2000"]
SOURCE_FLAGS = {"wavefront_primary.hip": ["-mllvm", "-structurizecfg-skip-uniform-regions=1"] + _WF_FLAGS,
                # (not the packet extend's option: it miscompiles the divergent shading code)
                "wavefront_primary_shade.hip": _WF_FLAGS,
                "wavefront.hip": _WF_FLAGS,
                # the lean LDS extend's body again: its flags
                "wavefront_sphere.hip": _WF_FLAGS,
                # ... and the extends' body with queue origins (the wavefront radiance queries)
                "wavefront_rays.hip": _WF_FLAGS,
                # the ray queries' kernel is the extend's loop: it starts from the extend's flags
                "rayquery.hip": _WF_FLAGS,
                # ... and the ambient-occlusion queries' is the ray queries' loop
                "ao.hip": _WF_FLAGS,
                # ... and the direct-lighting queries' is the ambient-occlusion queries'
                "direct.hip": _WF_FLAGS,
                "render.hip": ["-mllvm", "-enable-gvn-hoist", "-mllvm", "-unroll-threshold=2000"]}
# the machine scheduler where it is not the build's max-ILP one (wf_primary_shade: the
# register-minimising scheduler holds its 88-VGPR budget without scratch; MCPT_SCHED, the
# A/B variable, does not reach such a source -- any other scheduler gives it scratch)
SOURCE_SCHED = {"wavefront_primary_shade.hip": "iterative-minreg"}
HEADERS = ["capi_internal.hpp", "staging.hpp", "host_model.hpp", "mcpt_device.hpp", "render_launch.hpp", "stat_blocks.hpp", "wf_route.hpp", "trace_device.hpp", "half_box.hpp",
           "aov_device.hpp", "aov_launch.hpp", "variance_launch.hpp", "adaptive_launch.hpp", "partial_sum.hpp", "rayquery_launch.hpp", "ao_launch.hpp", "direct_launch.hpp", "temporal_launch.hpp",
           "wf_device.hpp", "wf_extend_body.hpp", "wf_primary_body.hpp", "wf_primary_walk.hpp", "wf_primary_pairs.hpp", "wf_primary_shade_body.hpp", "wf_shade_item.hpp"]
ARCH = os.environ.get("MCPT_OFFLOAD_ARCH", "gfx950")

COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-Wall",
          "-I" + os.path.join(ROOT, "include")] + os.environ.get("MCPT_EXTRA_FLAGS", "").split()


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(ROOT, "include", "mcpt.h"),
                                                                 os.path.abspath(__file__)]   # flags
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB
    os.makedirs(os.path.join(LIBDIR, "obj"), exist_ok=True)
    hipcc = _hipcc()

    def compile_one(src):
        obj = os.path.join(LIBDIR, "obj", os.path.basename(LIB) + "." + src + ".o")
        # max-ILP machine scheduling for the kernels: +1.2% C2, +1.5% C4, +0.9% wavefront
        # (the default occupancy-driven scheduler gains nothing: occupancy is fixed by LDS)
        sched = SOURCE_SCHED.get(src) or os.environ.get("MCPT_SCHED", "max-ilp")   # (the variable: A/B builds only)
        lang = (["-x", "hip", f"--offload-arch={ARCH}", "-mllvm", f"-amdgpu-sched-strategy={sched}"]
                if src.endswith(".hip")
                else ["-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"])
        cmd = [hipcc] + lang + COMMON + SOURCE_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"compile failed: {src}\n{r.stdout}\n{r.stderr}")
        return obj

    with ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    tmp = LIB + f".{os.getpid()}.tmp"
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed\n{r.stdout}\n{r.stderr}")
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
