"""Per-pixel variance and the variance-guided a-trous denoiser without a GPU: the
numpy restatement (tests/_var_ref.py) on oracle renders -- its rebuilt chunk
partial sums reproduce the oracle's spp_chunk render bit for bit, its variance
tracks the squared error against a converged render, and its guided filter
lowers the error where the plain one raises it; the C ABI's defaults, argument
checks and struct layout are checked through libmcpt.so.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _aov_ref as A
import _var_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
SEED = 0x4D435054
CASES = [(4, 1), (16, 2), (64, 8)]       # (spp, chunk)


@pytest.fixture(scope="module", autouse=True)
def entries(mcpt):
    """the restatement speaks for a library that has the entries it restates"""
    from montecarlopathtracer_amd._capi import lib
    for name in ("mcpt_render_var", "mcpt_render_var_device", "mcpt_denoise_var_params_default", "mcpt_denoise_var",
                 "mcpt_denoise_var_device"):
        assert getattr(lib(), name) is not None
    assert callable(mcpt.denoise_var) and callable(mcpt.Scene.render_var)


@pytest.fixture(scope="module")
def o_scene(mcpt, oracle_mod):
    return oracle_mod.Scene(mcpt.scene_path("scene01"))


@pytest.fixture(scope="module")
def converged(oracle_mod, o_scene):
    ref, _ = o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=2048, spp_offset=100000, threads=16))
    return ref


@pytest.fixture(scope="module")
def features(oracle_mod, o_scene):
    return A.aov_reference(oracle_mod, o_scene, W, H, 4, seed=SEED)


@pytest.fixture(scope="module")
def renders(oracle_mod, o_scene):
    """{(spp, chunk): (mean, var)} of the restatement fed with the oracle's chunk renders"""
    def chunk_render(n, off):
        return o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=n, spp_offset=off, seed=SEED,
                                                      threads=8))[0]
    out = {}
    for spp, chunk in CASES:
        out[(spp, chunk)] = V.variance(V.chunk_partials(chunk_render, spp, chunk), spp, chunk)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


# chunk lengths that are no powers of two (3 | 3 3 3 1 | 7 7 1 | 5 5 1 | 6 6): chunk_partials sums
# one-sample renders in order; spp_chunk 0 is one chunk of all samples (no variance, the mean only)
ODD_CASES = [(3, 0), (10, 3), (15, 7), (11, 5), (12, 6)]
_chunk_renders = {}


@pytest.mark.parametrize("spp,chunk", CASES + ODD_CASES)
def test_rebuilt_partials_reproduce_the_chunked_render(oracle_mod, o_scene, renders, spp, chunk):
    """sum of the rebuilt P_c / spp == the oracle's spp_chunk render, bit for bit"""
    ref, _ = o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, seed=SEED, threads=8))
    if (spp, chunk) in renders:
        assert np.array_equal(_bits(renders[(spp, chunk)][0]), _bits(ref))
        return

    def chunk_render(n, off):
        if (n, off) not in _chunk_renders:
            _chunk_renders[(n, off)] = o_scene.render(oracle_mod.RenderParams(
                width=W, height=H, spp=n, spp_offset=off, seed=SEED, threads=8))[0]
        return _chunk_renders[(n, off)]
    ns = V.chunk_lengths(spp, chunk or spp)
    assert any(n & (n - 1) for n in ns), ns                   # the one-sample route is taken
    parts = V.chunk_partials(chunk_render, spp, chunk or spp)
    total = np.zeros_like(parts[0])
    for P in parts:
        total = total + P
    mean = (total / np.float32(spp)).astype(np.float32)
    assert np.array_equal(_bits(mean), _bits(ref))
    if len(ns) >= 2:
        rmean, var = V.variance(parts, spp, chunk)
        assert np.array_equal(_bits(rmean), _bits(mean))
        assert np.isfinite(var).all() and (var >= 0).all() and var[..., :3].max() > 0


@pytest.mark.parametrize("spp,chunk", CASES)
def test_variance_tracks_the_squared_error(renders, converged, spp, chunk):
    mean, var = renders[(spp, chunk)]
    assert np.isfinite(var).all() and (var >= 0).all() and (var[..., 3] == 0).all()
    mv = float(var[..., :3].astype(np.float64).mean())
    mse = float(((mean.astype(np.float64) - converged.astype(np.float64)) ** 2).mean())
    print(f"spp {spp} chunk {chunk}: mean variance {mv:.5f} mean squared error {mse:.5f} ratio {mv / mse:.3f}")
    assert 0.5 <= mv / mse <= 2.0


def _ratios(oracle_mod, renders, converged, features, spp, chunk):
    mean, var = renders[(spp, chunk)]
    ac, nd = features
    e = _rmse(mean, converged)
    plain = _rmse(A.denoise(oracle_mod, mean, ac, nd), converged) / e
    guided = _rmse(V.denoise_var(oracle_mod, mean, var, ac, nd), converged) / e
    print(f"spp {spp} chunk {chunk}: RMSE noisy {e:.4f} plain ratio {plain:.3f} guided ratio {guided:.3f}")
    return plain, guided


def test_guided_filter_helps_at_64_spp_where_the_plain_one_hurts(oracle_mod, renders, converged, features):
    plain, guided = _ratios(oracle_mod, renders, converged, features, 64, 8)
    assert plain > 1.0
    assert guided < 0.95


def test_guided_filter_beats_the_plain_one_at_16_spp(oracle_mod, renders, converged, features):
    plain, guided = _ratios(oracle_mod, renders, converged, features, 16, 2)
    assert guided < plain


def test_guided_filter_lowers_the_error_at_4_spp(oracle_mod, renders, converged, features):
    _, guided = _ratios(oracle_mod, renders, converged, features, 4, 1)
    assert guided < 0.9


def test_unit_variance_and_a_huge_sigma_l_give_the_plain_filter(oracle_mod, renders, features):
    """every luminance weight rounds to exactly 1, so the RGB is _aov_ref.denoise's bit for bit"""
    mean, _ = renders[(4, 1)]
    ac, nd = features
    ones = np.ones((H, W, 4), np.float32)
    got = V.denoise_var(oracle_mod, mean, ones, ac, nd, sigma_l=1e30)
    ref = A.denoise(oracle_mod, mean, ac, nd)
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(ref))
    assert not np.array_equal(_bits(V.denoise_var(oracle_mod, mean, ones, ac, nd, sigma_l=0.01)), _bits(ref))


def test_zero_variance_keeps_equal_luminance_and_stays_finite(oracle_mod, features):
    """den = 1e-6 where the variance is 0: no division by zero, a flat image is a fixed point"""
    ac, nd = features
    flat = np.full((H, W, 3), 0.5, np.float32)
    out, a = V.denoise_var(oracle_mod, flat, np.zeros((H, W, 4), np.float32), ac, nd, return_variance=True)
    assert np.isfinite(out).all() and (a == 0).all()
    assert np.abs(out - flat).max() < 1e-6


# ---- the C ABI without a device ------------------------------------------------

def test_denoise_var_params_default(mcpt):
    from montecarlopathtracer_amd._capi import DenoiseParamsC, DenoiseVarParamsC, lib
    p = DenoiseVarParamsC(DenoiseParamsC(width=3, height=4, gamma_space=1), 9.0)
    lib().mcpt_denoise_var_params_default(C.byref(p))
    b = p.base
    assert (b.iterations, b.normal_power_log2, b.gamma_space) == (5, 7, 0)
    assert b.sigma_z == np.float32(0.1) and b.albedo_floor == np.float32(0.01)
    assert (b.width, b.height) == (0, 0)
    assert p.sigma_l == 4.0
    lib().mcpt_denoise_var_params_default(None)      # no-op
    q = mcpt.denoise_var_params(5, 6, sigma_l=2.5, iterations=3)
    assert (q.base.width, q.base.height, q.base.iterations, q.sigma_l) == (5, 6, 3, 2.5)


def test_denoise_var_invalid_arguments_fail_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import DenoiseParamsC, DenoiseVarParamsC, lib
    L = lib()
    n = 4 * 4
    col, var, a, nd, out = (np.zeros(n * k, np.float32) for k in (3, 4, 4, 4, 3))
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731

    def P(sigma_l=0.0, **kw):
        kw.setdefault("width", 4)
        kw.setdefault("height", 4)
        return DenoiseVarParamsC(DenoiseParamsC(**kw), sigma_l)

    def host(p, c=col, v=var, al=a, n_=nd, o=out):
        return L.mcpt_denoise_var(C.byref(p) if p is not None else None,
                                  *(fp(x) if x is not None else None for x in (c, v, al, n_, o)))

    assert host(None) == -1 and b"NULL" in L.mcpt_last_error()
    for missing in range(5):
        args = [col, var, a, nd, out]
        args[missing] = None
        assert host(P(), *args) == -1 and b"NULL" in L.mcpt_last_error()
    assert host(P(width=0)) == -1
    assert host(P(height=-1)) == -1
    assert host(P(iterations=9)) == -1 and b"iterations" in L.mcpt_last_error()
    assert host(P(sigma_z=-1.0)) == -1
    assert host(P(gamma_space=2)) == -1
    assert host(P(sigma_l=-0.5)) == -1 and b"sigma_l" in L.mcpt_last_error()
    assert host(P(sigma_l=float("nan"))) == -1 and b"sigma_l" in L.mcpt_last_error()
    # out aliasing an input, the variance among them
    assert host(P(), o=col) == -1 and b"overlap" in L.mcpt_last_error()
    big = np.zeros(n * 4, np.float32)
    assert host(P(), v=big, o=big) == -1 and b"overlap" in L.mcpt_last_error()
    assert host(P(), al=big, o=big) == -1
    # device entry: the same checks before any device call (the addresses are never dereferenced)
    vp = C.c_void_p
    dev = lambda p, *ptrs: L.mcpt_denoise_var_device(C.byref(p), *(vp(x) for x in ptrs), None)   # noqa: E731
    B = n * 16
    ptrs = [(1 << 20) + k * B for k in range(6)]     # colour, variance, albedo_cov, normal_depth, out, scratch
    assert L.mcpt_denoise_var_device(None, *(vp(x) for x in ptrs), None) == -1
    assert dev(P(iterations=9), *ptrs) == -1
    assert dev(P(sigma_l=-1.0), *ptrs) == -1 and b"sigma_l" in L.mcpt_last_error()
    for missing in range(6):
        q = list(ptrs)
        q[missing] = None
        assert dev(P(), *q) == -1 and b"NULL" in L.mcpt_last_error()
    for k in range(4):                                                     # out = an input
        assert dev(P(), *ptrs[:4], ptrs[k], ptrs[5]) == -1 and b"overlap" in L.mcpt_last_error()
    assert dev(P(), *ptrs[:4], ptrs[4], ptrs[4]) == -1                     # scratch = out
    assert dev(P(), *ptrs[:4], ptrs[4], ptrs[1] + 16) == -1                # scratch inside the variance
    with pytest.raises(mcpt.McptError) as e:
        z4 = np.zeros((4, 4, 4), np.float32)
        mcpt.denoise_var(np.zeros((4, 4, 3), np.float32), z4, z4, z4, sigma_l=-1.0)
    assert e.value.code == -1


def test_render_var_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    assert L.mcpt_render_var(None, None, None, None, None) == -1
    assert L.mcpt_render_var_device(None, None, None, None, None) == -1
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    fb = np.zeros((8, 8, 3), np.float32)
    var = np.zeros((8, 8, 4), np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    ok = mcpt.RenderParams(width=8, height=8, spp=4, spp_chunk=2)
    # NULL buffers and params
    assert L.mcpt_render_var(s.handle, C.byref(ok.to_c()), None, fp(var), None) == -1
    assert L.mcpt_render_var(s.handle, C.byref(ok.to_c()), fp(fb), None, None) == -1
    assert L.mcpt_render_var(s.handle, None, fp(fb), fp(var), None) == -1
    assert L.mcpt_render_var_device(s.handle, C.byref(ok.to_c()), None, C.c_void_p(1 << 21), None) == -1
    assert L.mcpt_render_var_device(s.handle, C.byref(ok.to_c()), C.c_void_p(1 << 20), None, None) == -1
    assert L.mcpt_render_var_device(s.handle, None, C.c_void_p(1 << 20), C.c_void_p(1 << 21), None) == -1
    # fewer than two chunks: spp_chunk 0 (the C default: one chunk), >= spp, or spp 1
    for kw in (dict(spp=4, spp_chunk=0), dict(spp=4, spp_chunk=4), dict(spp=4, spp_chunk=9), dict(spp=1, spp_chunk=1)):
        p = mcpt.RenderParams(width=8, height=8, **kw)
        with pytest.raises(mcpt.McptError) as e:
            s.render_var(p)
        assert e.value.code == -1 and "spp_chunk" in str(e.value), kw
        with pytest.raises(mcpt.McptError) as e:
            s.render_var_device(p, 1 << 20, 1 << 21)
        assert e.value.code == -1 and "spp_chunk" in str(e.value), kw
    # sharded, packed, RCCL gather: unsupported
    for kw in (dict(shard_count=2), dict(packed=True), dict(gather="rccl")):
        p = mcpt.RenderParams(width=8, height=8, spp=4, spp_chunk=2, **kw)
        with pytest.raises(mcpt.McptError) as e:
            s.render_var(p)
        assert e.value.code == -6, kw
        with pytest.raises(mcpt.McptError) as e:
            s.render_var_device(p, 1 << 20, 1 << 21)
        assert e.value.code == -6, kw
    # a host-only scene
    with pytest.raises(mcpt.McptError) as e:
        s.render_var(ok)
    assert e.value.code == -1 and "host-only" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.render_var_device(ok, 1 << 20, 1 << 21)
    assert e.value.code == -1 and "host-only" in str(e.value)
    # the framebuffer and the variance buffer may not overlap
    with pytest.raises(mcpt.McptError) as e:
        s.render_var_device(ok, 1 << 20, (1 << 20) + 16)
    assert "overlap" in str(e.value)
    with pytest.raises(mcpt.McptError):
        s.render_var(ok, var=np.zeros((8, 8, 3), np.float32))


def test_denoise_var_params_layout_matches_header(mcpt, tmp_path):
    """ctypes mirror of mcpt_denoise_var_params: sizes and offsets of include/mcpt.h"""
    from montecarlopathtracer_amd import _capi
    py = _capi.DenoiseVarParamsC
    assert [f for f, _ in py._fields_] == ["base", "sigma_l"]
    assert py.base.size == C.sizeof(_capi.DenoiseParamsC)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcpt.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(mcpt_denoise_var_params));',
             'printf("base_size %zu\\n", sizeof(mcpt_denoise_params));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(mcpt_denoise_var_params, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                         check=True).stdout.split("\n") if l)
    assert int(out["size"]) == C.sizeof(py)
    assert int(out["base_size"]) == C.sizeof(_capi.DenoiseParamsC)
    for f, _ in py._fields_:
        assert int(out[f]) == getattr(py, f).offset, f
