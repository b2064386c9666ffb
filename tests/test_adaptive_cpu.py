"""Variance-driven adaptive sampling without a GPU: the numpy restatement
(tests/_adaptive_ref.py) fed with the CPU oracle's per-pass images -- its result
is, pixel by pixel, the uniform chain of count[p] passes; every pass count
occurs (the coverage the GPU test relies on); at the default threshold it
reaches the error of more uniform samples than it spends -- and the C ABI's
defaults, struct layout, entries and argument checks through libmcpt.so.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _adaptive_ref as AR
import _var_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
SEED = 0x4D435054
S, CHUNK, PASSES = 8, 2, 8


@pytest.fixture(scope="module", autouse=True)
def entries(mcpt):
    """the restatement speaks for a library that has the entries it restates"""
    from montecarlopathtracer_amd._capi import lib
    for name in ("mcpt_adaptive_params_default", "mcpt_render_adaptive", "mcpt_render_adaptive_device"):
        assert getattr(lib(), name) is not None
    assert callable(mcpt.adaptive_params) and callable(mcpt.Scene.render_adaptive)
    assert callable(mcpt.Scene.render_adaptive_device)


@pytest.fixture(scope="module")
def o_scene(mcpt, oracle_mod):
    return oracle_mod.Scene(mcpt.scene_path("scene01"))


@pytest.fixture(scope="module")
def passes(oracle_mod, o_scene):
    """[(mean, var)] of the 8 passes of 8 spp in chunks of 2, from the oracle's chunk renders"""
    def chunk_render(n, off):
        return o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=n, spp_offset=off, seed=SEED,
                                                      threads=8))[0]
    return [V.variance(V.chunk_partials(chunk_render, S, CHUNK, spp_offset=j * S), S, CHUNK) for j in range(PASSES)]


@pytest.fixture(scope="module")
def chain(passes):
    return AR.uniform_chain(passes)


@pytest.fixture(scope="module")
def converged(oracle_mod, o_scene):
    ref, _ = o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=2048, spp_offset=100000, threads=16))
    return ref


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_uniform_chain_is_the_running_variance_of_the_variance_restatement(passes, chain):
    """merge() is csrc/variance.hip's blend: the chain equals V.variance fed with prev / prev_count"""
    assert np.array_equal(_bits(chain[0][0]), _bits(passes[0][0]))
    assert np.array_equal(_bits(chain[0][1]), _bits(passes[0][1]))
    # pass 1 through _var_ref's own blend (the partial sums are not kept: blend the plain variance)
    pc, pc1 = np.float32(1), np.float32(2)
    ref = ((chain[0][1][..., :3] * pc) * pc + passes[1][1][..., :3]) / (pc1 * pc1)
    assert np.array_equal(_bits(chain[1][1][..., :3]), _bits(ref))
    assert (chain[1][1][..., 3] == 0).all()


@pytest.mark.parametrize("dilate_r,histogram", [(1, [1202, 42, 41, 31, 7, 45, 42, 1662]),
                                                (0, [2710, 36, 30, 19, 9, 25, 16, 227])])
def test_adaptive_equals_the_uniform_chain_per_pixel_and_every_count_occurs(passes, chain, dilate_r, histogram):
    fb, var, count, active = AR.adaptive(passes, max_passes=PASSES, threshold=0.5, lum_floor=0.01, dilate_r=dilate_r)
    hist = np.bincount(count.ravel(), minlength=PASSES + 1)[1:].tolist()
    print("dilate", dilate_r, "count histogram", hist)
    assert count.min() >= 1 and count.max() <= PASSES
    for m in range(1, PASSES + 1):
        sel = count == m
        assert sel.any(), m                                   # the coverage the GPU test relies on
        assert np.array_equal(_bits(fb[sel]), _bits(chain[m - 1][0][sel])), m
        assert np.array_equal(_bits(var[sel]), _bits(chain[m - 1][1][sel])), m
    assert hist == histogram
    # monotone: pass j's pixels are a subset of pass j-1's, and count = passes a pixel was in
    for j in range(1, len(active)):
        assert not (active[j] & ~active[j - 1]).any()
    assert np.array_equal(count, np.sum(active, axis=0).astype(np.uint32))


@pytest.fixture(scope="module")
def odd_passes(oracle_mod, o_scene):
    """[(mean, var)] of 4 passes of 15 spp in chunks of 7, 7, 1: the partial sums of the 7-sample
    chunks are in-order sums of one-sample renders (_var_ref.chunk_partials), so P_c / 7 rounds"""
    def chunk_render(n, off):
        return o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=n, spp_offset=off, seed=SEED,
                                                      threads=8))[0]
    return [V.variance(V.chunk_partials(chunk_render, 15, 7, spp_offset=j * 15), 15, 7) for j in range(4)]


@pytest.mark.parametrize("dilate_r,histogram", [(1, [1032, 260, 97, 1683]), (0, [2612, 131, 71, 258])])
def test_adaptive_with_chunks_of_seven_equals_the_uniform_chain_per_pixel(oracle_mod, o_scene, odd_passes, dilate_r,
                                                                          histogram):
    chain = AR.uniform_chain(odd_passes)
    # the chain's first link is the oracle's own chunked render
    ref, _ = o_scene.render(oracle_mod.RenderParams(width=W, height=H, spp=15, spp_chunk=7, seed=SEED, threads=8))
    assert np.array_equal(_bits(chain[0][0]), _bits(ref))
    fb, var, count, active = AR.adaptive(odd_passes, max_passes=4, threshold=0.5, lum_floor=0.01, dilate_r=dilate_r)
    hist = np.bincount(count.ravel(), minlength=5)[1:].tolist()
    print("dilate", dilate_r, "count histogram", hist)
    for m in range(1, 5):
        sel = count == m
        assert sel.any(), m
        assert np.array_equal(_bits(fb[sel]), _bits(chain[m - 1][0][sel])), m
        assert np.array_equal(_bits(var[sel]), _bits(chain[m - 1][1][sel])), m
    assert hist == histogram
    assert np.array_equal(count, np.sum(active, axis=0).astype(np.uint32))


def test_min_passes_and_limits_of_the_restatement(passes, chain):
    _, _, count, _ = AR.adaptive(passes, max_passes=PASSES, min_passes=3, threshold=0.5)
    assert count.min() == 3 and count.max() == PASSES
    fb, var, count, _ = AR.adaptive(passes, max_passes=PASSES, threshold=1e30)
    assert (count == 1).all() and np.array_equal(_bits(fb), _bits(chain[0][0]))
    fb, var, count, _ = AR.adaptive(passes, max_passes=3, min_passes=3)
    assert (count == 3).all() and np.array_equal(_bits(fb), _bits(chain[2][0]))
    assert np.array_equal(_bits(var), _bits(chain[2][1]))


def test_adaptive_reaches_the_error_of_six_uniform_passes_with_fewer_samples(passes, chain, converged):
    """threshold 0.2, dilate 1.  Measured on the oracle: RMSE 0.0631 at 5.47 mean passes against
    0.0740 for the uniform 6-pass chain (0.0659 / 0.0631 for 7 / 8)."""
    fb, _, count, _ = AR.adaptive(passes, max_passes=PASSES, threshold=0.2, lum_floor=0.01, dilate_r=1)
    mean_count = float(count.mean())
    e, e6 = _rmse(fb, converged), _rmse(chain[5][0], converged)
    print(f"adaptive RMSE {e:.4f} at {mean_count:.2f} mean passes; uniform 6 / 7 / 8: {e6:.4f} / "
          f"{_rmse(chain[6][0], converged):.4f} / {_rmse(chain[7][0], converged):.4f}")
    assert mean_count <= 6.0
    assert e <= e6


# ---- the C ABI without a device ------------------------------------------------

def test_adaptive_params_default_and_layout(mcpt, tmp_path):
    from montecarlopathtracer_amd._capi import AdaptiveParamsC, lib
    p = AdaptiveParamsC(99, 99, 9.0, 9.0, 99, 99)
    lib().mcpt_adaptive_params_default(C.byref(p))
    assert (p.max_passes, p.min_passes, p.dilate, p.force_list) == (8, 1, 1, 0)
    assert p.threshold == np.float32(0.2) and p.lum_floor == np.float32(0.01)
    lib().mcpt_adaptive_params_default(None)      # no-op
    q = mcpt.adaptive_params(max_passes=5, min_passes=2, threshold=0.5, lum_floor=0.25, dilate=-1, force_list=True)
    assert (q.max_passes, q.min_passes, q.threshold, q.lum_floor, q.dilate, q.force_list) == (5, 2, 0.5, 0.25, -1, 1)
    z = mcpt.adaptive_params()
    assert (z.max_passes, z.min_passes, z.threshold, z.lum_floor, z.dilate, z.force_list) == (0, 0, 0.0, 0.0, 0, 0)
    names = ["max_passes", "min_passes", "threshold", "lum_floor", "dilate", "force_list"]
    assert [n for n, _ in AdaptiveParamsC._fields_] == names
    assert C.sizeof(AdaptiveParamsC) == 24
    assert [getattr(AdaptiveParamsC, n).offset for n in names] == [0, 4, 8, 12, 16, 20]
    assert lib().mcpt_abi_version() == 9
    # the header's own layout, where a C compiler is at hand
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mcpt.h"\nint main(void) {\n'
                       '  printf("%zu", sizeof(mcpt_adaptive_params));\n' +
                       "".join(f'  printf(" %zu", offsetof(mcpt_adaptive_params, {n}));\n' for n in names) +
                       '  printf(" %d", MCPT_ABI_VERSION);\n  return 0;\n}\n')
        exe = tmp_path / "layout"
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == [24, 0, 4, 8, 12, 16, 20, 9]


def test_render_adaptive_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    assert L.mcpt_render_adaptive(None, None, None, None, None, None, None) == -1
    assert L.mcpt_render_adaptive_device(None, None, None, None, None, None, None) == -1
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    fb = np.zeros((8, 8, 3), np.float32)
    var = np.zeros((8, 8, 4), np.float32)
    cnt = np.zeros((8, 8), np.uint32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    up = cnt.ctypes.data_as(C.POINTER(C.c_uint32))
    ok = mcpt.RenderParams(width=8, height=8, spp=4, spp_chunk=2)
    okc = ok.to_c()
    D = (1 << 20, 1 << 21, 1 << 22)                         # never dereferenced: every call fails first
    # NULL buffers and params
    assert L.mcpt_render_adaptive(s.handle, C.byref(okc), None, None, fp(var), up, None) == -1
    assert L.mcpt_render_adaptive(s.handle, C.byref(okc), None, fp(fb), None, up, None) == -1
    assert L.mcpt_render_adaptive(s.handle, C.byref(okc), None, fp(fb), fp(var), None, None) == -1
    assert L.mcpt_render_adaptive(s.handle, None, None, fp(fb), fp(var), up, None) == -1
    for k in range(3):
        q = [C.c_void_p(x) for x in D]
        q[k] = None
        assert L.mcpt_render_adaptive_device(s.handle, C.byref(okc), None, *q, None) == -1
        assert b"NULL" in L.mcpt_last_error()
    assert L.mcpt_render_adaptive_device(s.handle, None, None, *(C.c_void_p(x) for x in D), None) == -1

    def both(p, a, code, word):
        with pytest.raises(mcpt.McptError) as e:
            s.render_adaptive(p, a)
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
        with pytest.raises(mcpt.McptError) as e:
            s.render_adaptive_device(p, a, *D)
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))

    P = lambda **kw: mcpt.RenderParams(**{**dict(width=8, height=8, spp=4, spp_chunk=2), **kw})   # noqa: E731
    # everything mcpt_render_var rejects
    for kw in (dict(spp_chunk=0), dict(spp_chunk=4), dict(spp=1, spp_chunk=1)):
        both(P(**kw), None, -1, "spp_chunk")
    both(P(width=0), None, -1, "width")
    both(P(max_depth=-1), None, -1, "max_depth")
    # the adaptive render's own: a running mean of its own, the sample index range
    both(P(prev_count=1), None, -1, "prev_count")
    both(P(spp_offset=2 ** 32 - 31), mcpt.adaptive_params(), -1, "spp_offset")              # 8 x 4 = 32 samples
    both(P(spp=2 ** 20, spp_chunk=2 ** 19, spp_offset=1), mcpt.adaptive_params(max_passes=4096), -1, "max_passes")
    # adaptive fields out of range, each named
    for kw, word in ((dict(max_passes=-1), "max_passes"), (dict(max_passes=4097), "max_passes"),
                     (dict(min_passes=-1), "min_passes"), (dict(max_passes=4, min_passes=5), "min_passes"),
                     (dict(min_passes=9), "min_passes"),                                       # default max 8
                     (dict(threshold=-0.5), "threshold"), (dict(threshold=float("nan")), "threshold"),
                     (dict(lum_floor=-1.0), "lum_floor"), (dict(lum_floor=float("nan")), "lum_floor"),
                     (dict(dilate=5), "dilate")):
        both(P(), mcpt.adaptive_params(**kw), -1, word)
    bad = mcpt.adaptive_params()
    bad.force_list = 2
    both(P(), bad, -1, "force_list")
    # what mcpt_render_var refuses, and the adaptive render's own refusals
    for kw in (dict(shard_count=2), dict(packed=True), dict(gather="rccl")):
        both(P(**kw), None, -6, "")
    both(P(pipeline="wavefront"), None, -6, "pipeline")
    both(mcpt.RenderParams.for_quinengine(width=8, height=8, spp=4, spp_chunk=2), None, -6, "mode")
    # valid arguments reach the host-only scene
    both(ok, None, -1, "host-only")
    both(ok, mcpt.adaptive_params(max_passes=4096, min_passes=4096, threshold=1e30, dilate=4, force_list=True), -1,
         "host-only")
    both(P(spp_offset=2 ** 32 - 32), None, -1, "host-only")                                   # exactly 2^32: allowed
    # overlapping device buffers
    for ptrs in ((D[0], D[0] + 16, D[2]), (D[0], D[1], D[0] + 64), (D[0], D[1], D[1] + 1020)):
        with pytest.raises(mcpt.McptError) as e:
            s.render_adaptive_device(ok, None, *ptrs)
        assert "overlap" in str(e.value)
    with pytest.raises(mcpt.McptError):
        s.render_adaptive(ok, var=np.zeros((8, 8, 3), np.float32))
