"""Per-pixel variance of a render (csrc/variance.hip) and the variance-guided
a-trous denoiser (csrc/denoise_var.hip) on the GPU, bit for bit against their
numpy restatement (tests/_var_ref.py).  The variance kernel's chunk partial
sums are rebuilt from the GPU's own one-chunk renders (power-of-two chunk
lengths: mean * n is the partial sum exactly; any other length: the in-order
float32 sum of the chunk's one-sample renders); then the host and device
entries, the absence of side effects, and the public pipeline against a
converged render.
"""
import numpy as np
import pytest

import _var_ref as V

pytestmark = pytest.mark.gpu

_scenes = {}
_parts = {}
_chunk_renders = {}
INT_STATS = ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades", "stack_spills",
             "renders", "variant", "devices")


def _scene(mcpt, name="scene01", layout="auto"):
    if (name, layout) not in _scenes:
        flavor = "tinyobj" if name.startswith("qe_") else "cvmctracer"
        _scenes[(name, layout)] = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name), flavor=flavor), layout=layout)
    return _scenes[(name, layout)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equal(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(),
                           got[bad][:5].tolist(), ref[bad][:5].tolist())


def _partials(mcpt, W, H, spp, chunk, spp_offset=0):
    """chunk partial sums from the GPU's own one-chunk renders, computed once per frame (the
    one-sample renders of the chunk lengths that are no powers of two: once per frame and sample)"""
    key = (W, H, spp, chunk, spp_offset)
    if key not in _parts:
        scene = _scene(mcpt)

        def chunk_render(n, off):
            if (W, H, n, off) not in _chunk_renders:
                _chunk_renders[(W, H, n, off)] = scene.render(mcpt.RenderParams(width=W, height=H, spp=n,
                                                                                spp_offset=off))[0]
            return _chunk_renders[(W, H, n, off)]
        _parts[key] = V.chunk_partials(chunk_render, spp, chunk, spp_offset)
    return _parts[key]


def _packed_count(mcpt, W, H, tile):
    return len(mcpt.RenderParams(width=W, height=H, tile=tile, packed=True).shard_pixels())


VAR_CASES = [
    # id, W, H, spp, chunk, scene layout, render params
    ("defaults", 64, 48, 16, 2, "auto", {}),                                 # every unit through the tail buffer
    ("no-tail-split", 64, 48, 16, 2, "auto", dict(tail_units_per_lane=-1)),  # every unit a plain partial sum
    ("mixed-tail", 64, 48, 16, 2, "auto", dict(tail_units=5000)),            # both kinds in one frame
    ("wavefront", 64, 48, 16, 2, "auto", dict(pipeline="wavefront")),
    ("global-layout", 64, 48, 16, 2, "global", {}),
    ("ragged-37x29", 37, 29, 12, 4, "auto", {}),                             # tile padding, three chunks
    ("short-last-chunk", 64, 48, 10, 4, "auto", {}),                         # chunks of 4, 4, 2
    ("more-pixels-than-lanes", 608, 440, 2, 1, "auto", {}),
    # packed pixel counts (owned tiles x tile^2) that are no multiples of 256 -- or of 64: the
    # variance kernel's last workgroup and wave are partly filled; an eighth field = that count
    ("tile1-37x29", 37, 29, 6, 2, "auto", dict(tile=1), 1073),
    ("tile4-36x28", 36, 28, 6, 2, "auto", dict(tile=4), 1008),
    ("tile5-37x29", 37, 29, 6, 2, "auto", dict(tile=5), 1200),
    ("three-waves-24x8", 24, 8, 8, 2, "auto", {}, 192),
    ("one-wave-8x8", 8, 8, 8, 2, "auto", {}, 64),
    # one real pixel in a wave of padding; samples 48..55 are the first with radiance in it (oracle)
    ("one-pixel-1x1", 1, 1, 8, 2, "auto", dict(spp_offset=48), 64),
]
# chunk lengths that are no powers of two (3 3 3 1 | 7 7 1 | 5 5 1 | 6 6): d = P_c / n - mean rounds
ODD_CHUNKS = [(10, 3), (15, 7), (11, 5), (12, 6)]
ODD_VARIANTS = [("defaults", "auto", {}), ("no-tail-split", "auto", dict(tail_units_per_lane=-1)),
                ("mixed-tail", "auto", dict(tail_units=5000)), ("wavefront", "auto", dict(pipeline="wavefront")),
                ("global-layout", "global", {})]
VAR_CASES += [(f"spp{s}-chunk{c}-{name}", 64, 48, s, c, layout, kw) for s, c in ODD_CHUNKS
              for name, layout, kw in ODD_VARIANTS]


@pytest.mark.parametrize("case", VAR_CASES, ids=lambda c: c[0])
def test_render_var_equals_render_and_restatement(mcpt, case):
    _, W, H, spp, chunk, layout, kw = case[:7]
    if len(case) > 7:
        npk = _packed_count(mcpt, W, H, kw.get("tile", 8))
        assert npk == case[7] and npk % 256 != 0
        assert npk % 64 != 0 or kw.get("tile", 8) == 8
    if (spp, chunk) in ODD_CHUNKS:
        assert any(n & (n - 1) for n in V.chunk_lengths(spp, chunk))
        if "tail_units" in kw:
            assert 0 < kw["tail_units"] < W * H * len(V.chunk_lengths(spp, chunk))   # both kinds of unit
    scene = _scene(mcpt, layout=layout)
    if layout == "global":
        assert int(scene.info()["node_boxes"]) == 1
    p = mcpt.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, **kw)
    ref_fb, ref_st = scene.render(p)
    fb, var, st = scene.render_var(p)
    _assert_equal(fb, ref_fb, "framebuffer")
    assert {k: st[k] for k in INT_STATS} == {k: ref_st[k] for k in INT_STATS}
    mean, ref_var = V.variance(_partials(mcpt, W, H, spp, chunk, kw.get("spp_offset", 0)), spp, chunk)
    _assert_equal(mean, ref_fb, "restated mean")          # the rebuilt partial sums are the render's
    assert var.shape == (H, W, 4) and (var[..., 3] == 0).all() and var[..., :3].max() > 0
    _assert_equal(var, ref_var, "variance")


def test_render_var_running_variance_over_two_calls(mcpt):
    scene = _scene(mcpt)
    W, H, spp, chunk = 37, 29, 8, 2
    fb, var, _ = scene.render_var(mcpt.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk))
    fb1, var1 = fb.copy(), var.copy()
    p2 = mcpt.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, spp_offset=spp, prev_count=1)
    scene.render_var(p2, fb, var)
    _, r1 = V.variance(_partials(mcpt, W, H, spp, chunk), spp, chunk)
    _assert_equal(var1, r1, "first variance")
    _, r2 = V.variance(_partials(mcpt, W, H, spp, chunk, spp_offset=spp), spp, chunk, prev=r1, prev_count=1)
    assert not np.array_equal(r2, r1)
    _assert_equal(var, r2, "running variance")
    ref_fb, _ = scene.render(p2, fb1.copy())
    _assert_equal(fb, ref_fb, "running mean")


def test_render_var_running_variance_over_two_calls_with_chunks_of_seven(mcpt):
    scene = _scene(mcpt)
    W, H, spp, chunk = 64, 48, 15, 7
    fb, var, _ = scene.render_var(mcpt.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk))
    fb1, var1 = fb.copy(), var.copy()
    p2 = mcpt.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, spp_offset=spp, prev_count=1)
    scene.render_var(p2, fb, var)
    _, r1 = V.variance(_partials(mcpt, W, H, spp, chunk), spp, chunk)
    _assert_equal(var1, r1, "first variance")
    m2, r2 = V.variance(_partials(mcpt, W, H, spp, chunk, spp_offset=spp), spp, chunk, prev=r1, prev_count=1)
    assert not np.array_equal(r2, r1)
    _assert_equal(var, r2, "running variance")
    _assert_equal(fb, ((fb1 * np.float32(1) + m2) / np.float32(2)).astype(np.float32), "running mean, restated")
    ref_fb, _ = scene.render(p2, fb1.copy())
    _assert_equal(fb, ref_fb, "running mean")


def test_render_var_quinengine_mode(mcpt):
    scene = _scene(mcpt, "qe_scene01")
    p = mcpt.RenderParams.for_quinengine(width=64, height=48, spp=8, spp_chunk=2, seed=822569775)
    ref_fb, _ = scene.render(p)
    fb, var, _ = scene.render_var(p)
    _assert_equal(fb, ref_fb, "framebuffer")
    assert np.isfinite(var).all() and (var >= 0).all() and var[..., :3].max() > 0 and (var[..., 3] == 0).all()


def test_render_var_host_and_device_entries_agree_without_side_effects(mcpt):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    p = mcpt.RenderParams(width=48, height=32, spp=4, spp_chunk=2)
    d_fb = torch.full((p.height, p.width, 4), -1.0, device="cuda")
    d_var = torch.full((p.height, p.width, 4), -1.0, device="cuda")
    torch.cuda.synchronize()
    scene.reserve(p)
    free0 = scene.plan(p)["device_free_bytes"]
    scene.render_var_device(p, d_fb.data_ptr(), d_var.data_ptr())       # after a reserve: no allocation
    torch.cuda.synchronize()
    assert scene.plan(p)["device_free_bytes"] == free0
    scene.stats()                                                       # a fresh record
    before, st0 = scene.render(p)
    fb, var, st1 = scene.render_var(p)
    _assert_equal(d_fb.cpu().numpy()[..., :3], fb, "device vs host framebuffer")
    _assert_equal(d_var.cpu().numpy(), var, "device vs host variance")
    _assert_equal(fb, before, "framebuffer")
    after, st2 = scene.render(p)                                        # a later plain render: the same bits
    _assert_equal(after, before, "render after render_var")
    assert st0["renders"] == st1["renders"] == st2["renders"] == 1 and st0["rays"] == st1["rays"] == st2["rays"]
    with pytest.raises(mcpt.McptError) as e:                            # one chunk: no variance
        scene.render_var(mcpt.RenderParams(width=48, height=32, spp=4, spp_chunk=4))
    assert e.value.code == -1 and "spp_chunk" in str(e.value)
    for kw in (dict(shard_count=2), dict(packed=True), dict(gather="rccl")):
        with pytest.raises(mcpt.McptError) as e:
            scene.render_var(mcpt.RenderParams(width=48, height=32, spp=4, spp_chunk=2, **kw))
        assert e.value.code == -6


# ---- the variance-guided filter ---------------------------------------------------

@pytest.fixture(scope="module")
def real_inputs(mcpt):
    """(colour, variance, albedo_cov, normal_depth) of scene01 at 64x48"""
    scene = _scene(mcpt)
    fb, var, _ = scene.render_var(mcpt.RenderParams(width=64, height=48, spp=16, spp_chunk=2))
    ac, nd = scene.render_aov(mcpt.RenderParams(width=64, height=48, spp=4))
    return fb, var, ac, nd


@pytest.mark.parametrize("iterations", [1, 5])
def test_denoise_var_equals_restatement_on_real_inputs(mcpt, oracle_mod, real_inputs, iterations):
    fb, var, ac, nd = real_inputs
    got = mcpt.denoise_var(fb, var, ac, nd, iterations=iterations)
    ref = V.denoise_var(oracle_mod, fb, var, ac, nd, iterations=iterations)
    assert np.isfinite(got).all() and not np.array_equal(got, fb)
    _assert_equal(got, ref, f"denoise_var x{iterations}")
    assert not np.array_equal(got, mcpt.denoise(fb, ac, nd, iterations=iterations))


def _random_inputs(rng, H, W):
    n = rng.standard_normal((H, W, 3)).astype(np.float32) + np.float32(3) * np.array([0, 0, 1], np.float32)
    n = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(np.float32)
    z = rng.uniform(4.0, 6.0, (H, W, 1)).astype(np.float32)
    alb = rng.random((H, W, 3)).astype(np.float32) ** 3          # some below the albedo floor
    ac = np.concatenate([alb, np.ones((H, W, 1), np.float32)], -1).astype(np.float32)
    nd = np.concatenate([n, z], -1).astype(np.float32)
    miss = rng.random((H, W)) < 0.1                               # miss pixels: all-zero features
    ac[miss] = 0
    nd[miss] = 0
    var = np.zeros((H, W, 4), np.float32)
    var[..., :3] = (rng.random((H, W, 3)) * 0.05).astype(np.float32)
    var[:, : W // 3] = 0                                          # a zero-variance region
    var[H // 2, W // 2, :3] = -1.0                                # clamped to 0
    color = (0.5 + 0.2 * rng.standard_normal((H, W, 3))).astype(np.float32)
    color[:, : W // 3] = np.float32(0.5)                          # flat where the variance is 0
    return color, var, ac, nd


def test_denoise_var_equals_restatement_on_random_inputs_8_iterations(mcpt, oracle_mod):
    H, W = 29, 37
    color, var, ac, nd = _random_inputs(np.random.default_rng(11), H, W)
    kw = dict(iterations=8, normal_power_log2=2, sigma_z=0.5, albedo_floor=0.05, sigma_l=2.0)
    got = mcpt.denoise_var(color, var, ac, nd, **kw)
    assert np.isfinite(got).all()
    _assert_equal(got, V.denoise_var(oracle_mod, color, var, ac, nd, **kw), "denoise_var x8")
    assert np.abs(got - color).max() > 1e-3


@pytest.mark.parametrize("H,W", [(1, 1), (1, 17), (17, 1), (16, 16), (17, 33)], ids=lambda v: str(v))
def test_denoise_var_at_degenerate_sizes(mcpt, oracle_mod, H, W):
    """one pixel, one row, one column, one 16x16 workgroup, one more than two: at 5 iterations the
    steps of 8 and 16 reach past every such frame (at 1x1 only the centre tap is left), and the
    3x3 variance prefilter loses its taps outside the image"""
    color, var, ac, nd = _random_inputs(np.random.default_rng(100 * H + W), H, W)
    kw = dict(iterations=5, normal_power_log2=2, sigma_z=0.5, sigma_l=2.0)
    got = mcpt.denoise_var(color, var, ac, nd, **kw)
    assert got.shape == (H, W, 3) and np.isfinite(got).all()
    _assert_equal(got, V.denoise_var(oracle_mod, color, var, ac, nd, **kw), f"denoise_var {W}x{H}")
    if H * W > 1:
        assert np.abs(got - color).max() > 1e-3


def test_denoise_var_gamma_space(mcpt, oracle_mod, real_inputs):
    H, W = 20, 24
    _, var, ac, nd = (np.ascontiguousarray(a[:H, :W]) for a in real_inputs)
    color = np.random.default_rng(3).random((H, W, 3)).astype(np.float32)
    got = mcpt.denoise_var(color, var, ac, nd, gamma_space=True)
    _assert_equal(got, V.denoise_var(oracle_mod, color, var, ac, nd, gamma_space=True), "gamma")
    assert not np.array_equal(got, mcpt.denoise_var(color, var, ac, nd))


def test_denoise_var_with_unit_variance_and_huge_sigma_l_is_the_plain_filter(mcpt, real_inputs):
    fb, _, ac, nd = real_inputs
    ones = np.ones((48, 64, 4), np.float32)
    _assert_equal(mcpt.denoise_var(fb, ones, ac, nd, sigma_l=1e30), mcpt.denoise(fb, ac, nd), "identity")


def test_denoise_var_host_and_device_entries_agree_and_repeat(mcpt, real_inputs):
    import torch
    fb, var, ac, nd = real_inputs
    H, W = fb.shape[:2]
    host = mcpt.denoise_var(fb, var, ac, nd, iterations=4)
    rgba = np.concatenate([fb, np.full((H, W, 1), 7.0, np.float32)], -1)        # the colour's alpha is ignored
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rgba, var, ac, nd)]
    ptrs = [x.data_ptr() for x in t]
    outs = []
    for _ in range(2):
        out = torch.full((H, W, 4), -1.0, device="cuda")
        scratch = torch.full((H, W, 4), -1.0, device="cuda")
        mcpt.denoise_var_device(W, H, *ptrs, out.data_ptr(), scratch.data_ptr(), iterations=4)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(t[0].cpu().numpy(), rgba) and np.array_equal(t[1].cpu().numpy(), var)   # inputs only read
    _assert_equal(outs[0], outs[1], "two runs")
    _assert_equal(outs[0][..., :3], host, "device vs host")
    assert (outs[0][..., 3] == 0).all()                                          # output alpha 0
    out = torch.zeros((H, W, 4), device="cuda")
    for bad_out, bad_scratch in ((ptrs[0], out.data_ptr()), (ptrs[1], out.data_ptr()), (out.data_ptr(), ptrs[1]),
                                 (out.data_ptr(), out.data_ptr())):
        with pytest.raises(mcpt.McptError) as e:                                 # out / scratch aliasing
            mcpt.denoise_var_device(W, H, *ptrs, bad_out, bad_scratch)
        assert "overlap" in str(e.value)


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_render_var_denoise_var_lowers_the_error_where_the_plain_filter_raises_it(mcpt):
    """The public pipeline at 64 spp against a converged 1024-spp render of other samples."""
    scene = _scene(mcpt)
    W, H = 64, 48
    ref, _ = scene.render(mcpt.RenderParams(width=W, height=H, spp=1024, spp_offset=100000))
    noisy, var, _ = scene.render_var(mcpt.RenderParams(width=W, height=H, spp=64, spp_chunk=8))
    ac, nd = scene.render_aov(mcpt.RenderParams(width=W, height=H, spp=4))
    e = _rmse(noisy, ref)
    plain = _rmse(mcpt.denoise(noisy, ac, nd), ref) / e
    guided = _rmse(mcpt.denoise_var(noisy, var, ac, nd), ref) / e
    print(f"RMSE noisy {e:.4f} plain ratio {plain:.3f} guided ratio {guided:.3f}")
    assert plain > 1.0
    assert guided < 0.95
