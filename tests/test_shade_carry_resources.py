"""Resource pins for the queue-order shade's terminal cull and carry (no GPU
needed), read from the built library's code objects as test_kernel_resources.py
does: all four 512-thread shade variants -- the ones that run beside an LDS
extend workgroup, two waves per SIMD in the 160 VGPRs it leaves -- at <= 80
VGPRs without scratch, and the kernels the change must not touch -- the lean
LDS extend, wf_primary_lists, wf_tile_candidates -- instruction for instruction
the code of the commit before it: tests/golden/shade_carry_isa.json holds the
SHA-256 of each one's instruction stream (scripts/isa_diff.py's normal form:
addresses and branch offsets stripped) from that commit's library, built with
the same toolchain.  A toolchain change moves these hashes without any change
of the source: re-record them from a build of the unchanged kernels then.
"""
import hashlib
import json
import os
import re
import sys

import pytest

from test_kernel_resources import LLVM, ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shade_carry_isa.json")
UNTOUCHED = r"wf_extendILi1ELi4ELi1024ELb0EE|wf_primary_lists|wf_tile_candidates"


def isa_hashes(lib):
    from isa_diff import kernel_text
    text, res = kernel_text(lib)
    return {n: hashlib.sha256("\n".join(text[n]).encode()).hexdigest() for n in res if re.search(UNTOUCHED, n)}, res


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("ROCm llvm tools not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return isa_hashes(b.build())                    # no-op when libmcpt.so is up to date


def test_shades_beside_the_lds_extend_fit_two_waves_per_simd(built):
    _, res = built
    shade = {k: r for k, r in res.items() if re.search(r"wf_shade_slotsILi512E", k)}
    assert len(shade) == 4, sorted(shade)           # (material table in LDS or not) x (queue order, sorted)
    for name, r in shade.items():
        assert r["vgpr"] + r["agpr"] <= 80 and r["scratch"] == 0, (name, r)


def test_untouched_kernels_keep_their_code(built):
    hashes, _ = built
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want) >= 3 and set(hashes) == set(want), sorted(set(hashes) ^ set(want))
    moved = [n for n in want if hashes[n] != want[n]]
    assert not moved, "instruction streams differ from the recorded ones (source change, or a new toolchain): %s" % moved
