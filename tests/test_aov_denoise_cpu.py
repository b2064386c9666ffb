"""First-hit feature buffers and the a-trous denoiser without a GPU: the numpy
restatement (tests/_aov_ref.py) is tied to the oracle -- its primary rays and
first hits reproduce the oracle's max_depth = 0 render bit for bit -- and its
denoiser lowers the error of noisy oracle renders; the C ABI's defaults,
argument checks and struct layout are checked through libmcpt.so.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _aov_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def o_scene(mcpt, oracle_mod):
    return oracle_mod.Scene(mcpt.scene_path("scene01"))


@pytest.mark.parametrize("W,H,spp,seed", [(64, 48, 4, 0x4D435054), (37, 29, 5, 12345)])
def test_helper_emission_equals_oracle_depth0_render(oracle_mod, o_scene, W, H, spp, seed):
    """Ka * illum at the helper's first hits == orc_render(max_depth=0): the helper's
    primary rays (also at a non-power-of-two width) and hits are the render's."""
    ref, _ = o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=spp, max_depth=0, seed=seed, threads=8))
    o, d = R.primary_rays(oracle_mod, W, H, spp, seed=seed)
    hits = R.first_hits(oracle_mod, o_scene, o, d)
    got = R.emission(o_scene, hits)
    assert hits["hit"].mean() > 0.5 and ref.max() > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.fixture(scope="module")
def converged(oracle_mod, o_scene):
    ref, _ = o_scene.render(oracle_mod.RenderParams(width=64, height=48, spp=2048, spp_offset=100000, threads=16))
    return ref


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("spp,seed", [(4, 0x4D435054), (1, 1)])
def test_numpy_denoiser_lowers_the_error(oracle_mod, o_scene, converged, spp, seed):
    W, H = 64, 48
    noisy, _ = o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=spp, seed=seed, threads=8))
    ac, nd = R.aov_reference(oracle_mod, o_scene, W, H, spp, seed=seed)
    den = R.denoise(oracle_mod, noisy, ac, nd)
    e_noisy, e_den = _rmse(noisy, converged), _rmse(den, converged)
    print(f"spp {spp} seed {seed}: RMSE noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
    assert np.isfinite(den).all()
    assert e_den < e_noisy


def test_denoise_params_default(mcpt):
    from montecarlopathtracer_amd._capi import DenoiseParamsC, lib
    p = DenoiseParamsC(width=3, height=4, gamma_space=1)
    lib().mcpt_denoise_params_default(C.byref(p))
    assert (p.iterations, p.normal_power_log2, p.gamma_space) == (5, 7, 0)
    assert p.sigma_z == np.float32(0.1) and p.albedo_floor == np.float32(0.01)
    assert (p.width, p.height) == (0, 0)
    lib().mcpt_denoise_params_default(None)      # no-op


def test_invalid_arguments_fail_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import DenoiseParamsC, lib
    L = lib()
    n = 4 * 4
    col, a, nd, out = (np.zeros(n * k, np.float32) for k in (3, 4, 4, 3))
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    ok = dict(width=4, height=4)

    def host(p, c=col, al=a, n_=nd, o=out):
        return L.mcpt_denoise(C.byref(p) if p is not None else None, *(fp(x) if x is not None else None
                                                                          for x in (c, al, n_, o)))

    assert host(None) == -1 and b"NULL" in L.mcpt_last_error()
    for missing in range(4):
        args = [col, a, nd, out]
        args[missing] = None
        assert host(DenoiseParamsC(**ok), *args) == -1
    assert host(DenoiseParamsC(width=0, height=4)) == -1
    assert host(DenoiseParamsC(width=4, height=-1)) == -1
    assert host(DenoiseParamsC(iterations=9, **ok)) == -1 and b"iterations" in L.mcpt_last_error()
    assert host(DenoiseParamsC(iterations=-1, **ok)) == -1
    assert host(DenoiseParamsC(normal_power_log2=11, **ok)) == -1
    assert host(DenoiseParamsC(sigma_z=-1.0, **ok)) == -1
    assert host(DenoiseParamsC(gamma_space=2, **ok)) == -1
    # out aliasing an input
    assert host(DenoiseParamsC(**ok), o=col) == -1 and b"overlap" in L.mcpt_last_error()
    big = np.zeros(n * 4, np.float32)
    assert host(DenoiseParamsC(**ok), al=big, o=big) == -1
    # device entry: the same checks before any device call (the addresses are never dereferenced)
    vp = C.c_void_p
    dev = lambda p, *ptrs: L.mcpt_denoise_device(C.byref(p), *(vp(x) for x in ptrs), None)   # noqa: E731
    B = n * 16
    base = 1 << 20
    ptrs = [base + k * B for k in range(5)]
    assert dev(DenoiseParamsC(iterations=9, **ok), *ptrs) == -1
    assert dev(DenoiseParamsC(**ok), ptrs[0], ptrs[1], ptrs[2], None, ptrs[4]) == -1
    assert dev(DenoiseParamsC(**ok), ptrs[0], ptrs[1], ptrs[2], ptrs[0], ptrs[4]) == -1        # out = colour
    assert dev(DenoiseParamsC(**ok), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[3]) == -1        # scratch = out
    assert dev(DenoiseParamsC(**ok), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[2] + 16) == -1   # scratch in normal_depth
    # the AOV entries
    assert L.mcpt_render_aov(None, None, None, None) == -1
    assert L.mcpt_render_aov_device(None, None, None, None, None) == -1
    with pytest.raises(mcpt.McptError) as e:
        mcpt.denoise(np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32),
                     iterations=9)
    assert e.value.code == -1


def test_denoise_params_layout_matches_header(mcpt, tmp_path):
    """ctypes mirror of mcpt_denoise_params: sizes and offsets of include/mcpt.h (as
    tests/test_capi.py test_struct_layouts_match_header does for the other structs)."""
    from montecarlopathtracer_amd import _capi
    py = _capi.DenoiseParamsC
    assert [f for f, _ in py._fields_] == ["width", "height", "iterations", "normal_power_log2", "sigma_z",
                                           "albedo_floor", "gamma_space"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcpt.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(mcpt_denoise_params));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(mcpt_denoise_params, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                         check=True).stdout.split("\n") if l)
    assert int(out["size"]) == C.sizeof(py)
    for f, _ in py._fields_:
        assert int(out[f]) == getattr(py, f).offset, f


def test_render_aov_on_a_host_only_scene_fails(mcpt):
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    with pytest.raises(mcpt.McptError) as e:
        s.render_aov(mcpt.RenderParams(width=8, height=8, spp=1))
    assert e.value.code == -1 and "host-only" in str(e.value)
    # the device entry: the same check, before any device call
    with pytest.raises(mcpt.McptError) as e:
        s.render_aov_device(mcpt.RenderParams(width=8, height=8, spp=1), 1 << 20, 1 << 21)
    assert "host-only" in str(e.value)
