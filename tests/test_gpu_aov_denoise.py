"""First-hit feature buffers (csrc/aov.hip) and the a-trous denoiser
(csrc/denoise.hip) on the GPU, bit for bit against their numpy restatement
(tests/_aov_ref.py: the oracle's RNG, camera, pow and ordered KD walk), through
the host and the device entries; then the public pipeline render -> features
-> denoise against a converged render, and the absence of side effects on the
scene's renders, statistics and memory.
"""
import numpy as np
import pytest

import _aov_ref as R

pytestmark = pytest.mark.gpu

_scenes = {}


def _scene(mcpt, oracle_mod, name):
    """(product scene, oracle scene, node_boxes), one per scene for the module"""
    if name not in _scenes:
        flavor = "tinyobj" if name.startswith("qe_") else "cvmctracer"
        path = mcpt.scene_path(name)
        s = mcpt.Scene(mcpt.ObjModel(path, flavor=flavor))
        _scenes[name] = (s, oracle_mod.Scene(path, flavor=flavor), int(s.info()["node_boxes"]))
    return _scenes[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equal(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(),
                           got[bad][:5].tolist(), ref[bad][:5].tolist())


AOV_CASES = [
    # scene, W, H, spp, seed, fresnel_kd, eye
    ("scene01", 64, 48, 4, 0x4D435054, True, (0.0, 5.0, 17.0)),
    ("scene01", 37, 29, 5, 12345, False, (0.0, 5.0, 17.0)),      # ragged tile edge, non-power-of-two width
    ("scene03", 40, 30, 2, 0x4D435054, True, (0.0, 5.0, 23.0)),  # global-memory layout, child-box cull
    ("scene01", 608, 440, 1, 7, True, (0.0, 5.0, 17.0)),         # more pixels than launched lanes: the lane stride
]


@pytest.mark.parametrize("case", AOV_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}")
def test_aov_equals_restatement(mcpt, oracle_mod, case):
    name, W, H, spp, seed, fkd, eye = case
    scene, o_scene, boxes = _scene(mcpt, oracle_mod, name)
    if name == "scene03":
        assert boxes == 1
    ac, nd = scene.render_aov(mcpt.RenderParams(width=W, height=H, spp=spp, seed=seed, fresnel_kd=fkd, eye=eye))
    rac, rnd = R.aov_reference(oracle_mod, o_scene, W, H, spp, node_boxes=boxes, fresnel_kd=fkd, seed=seed, eye=eye)
    assert 0.25 < ac[..., 3].mean() <= 1.0 and (nd[..., 3] >= 0).all()
    _assert_equal(ac, rac, "albedo_cov")
    _assert_equal(nd, rnd, "normal_depth")


def test_aov_quinengine_mode(mcpt, oracle_mod):
    scene, o_scene, boxes = _scene(mcpt, oracle_mod, "qe_scene01")
    W, H, spp, seed = 40, 24, 3, 822569775
    ac, nd = scene.render_aov(mcpt.RenderParams.for_quinengine(width=W, height=H, spp=spp, seed=seed))
    rac, rnd = R.aov_reference(oracle_mod, o_scene, W, H, spp, mode="qe", node_boxes=boxes, fresnel_kd=False,
                               seed=seed)
    assert ac[..., 3].mean() > 0.5
    _assert_equal(ac, rac, "albedo_cov")
    _assert_equal(nd, rnd, "normal_depth")


def test_aov_running_mean_over_two_calls(mcpt, oracle_mod):
    scene, o_scene, boxes = _scene(mcpt, oracle_mod, "scene01")
    W, H, spp = 37, 29, 2
    ac, nd = scene.render_aov(mcpt.RenderParams(width=W, height=H, spp=spp))
    first = (ac.copy(), nd.copy())
    scene.render_aov(mcpt.RenderParams(width=W, height=H, spp=spp, spp_offset=spp, prev_count=1), ac, nd)
    r1 = R.aov_reference(oracle_mod, o_scene, W, H, spp, node_boxes=boxes)
    _assert_equal(first[0], r1[0], "first albedo_cov")
    r2 = R.aov_reference(oracle_mod, o_scene, W, H, spp, node_boxes=boxes, spp_offset=spp, prev=r1, prev_count=1)
    assert not np.array_equal(r2[1], r1[1])
    _assert_equal(ac, r2[0], "albedo_cov")
    _assert_equal(nd, r2[1], "normal_depth")


def _aov_device(mcpt, scene, p):
    import torch
    ac = torch.zeros((p.height, p.width, 4), device="cuda")
    nd = torch.zeros((p.height, p.width, 4), device="cuda")
    scene.render_aov_device(p, ac.data_ptr(), nd.data_ptr())
    torch.cuda.synchronize()
    return ac, nd


def test_aov_host_and_device_entries_agree(mcpt, oracle_mod):
    scene, _, _ = _scene(mcpt, oracle_mod, "scene01")
    p = mcpt.RenderParams(width=37, height=29, spp=3, seed=99)
    ac, nd = scene.render_aov(p)
    dac, dnd = _aov_device(mcpt, scene, p)
    _assert_equal(dac.cpu().numpy(), ac, "albedo_cov")
    _assert_equal(dnd.cpu().numpy(), nd, "normal_depth")
    # sharded or packed feature buffers are refused
    for kw in (dict(shard_count=2), dict(packed=True)):
        with pytest.raises(mcpt.McptError) as e:
            scene.render_aov(mcpt.RenderParams(width=16, height=16, spp=1, **kw))
        assert e.value.code == -6


@pytest.fixture(scope="module")
def real_features(mcpt, oracle_mod):
    scene, _, _ = _scene(mcpt, oracle_mod, "scene01")
    return scene.render_aov(mcpt.RenderParams(width=37, height=29, spp=5, seed=12345))


@pytest.mark.parametrize("iterations", [1, 5])   # at 5 the step of 16 reaches past the image
def test_denoise_equals_restatement_on_real_features(mcpt, oracle_mod, real_features, iterations):
    ac, nd = real_features
    color = (np.random.default_rng(5).random((29, 37, 3)) * 2.0).astype(np.float32)
    got = mcpt.denoise(color, ac, nd, iterations=iterations)
    ref = R.denoise(oracle_mod, color, ac, nd, iterations=iterations)
    assert np.isfinite(got).all() and not np.array_equal(got, color)
    _assert_equal(got, ref, f"denoise x{iterations}")


def _random_features(rng, H, W):
    n = rng.standard_normal((H, W, 3)).astype(np.float32)
    n = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(np.float32)
    z = rng.uniform(1.0, 20.0, (H, W, 1)).astype(np.float32)
    alb = rng.random((H, W, 3)).astype(np.float32) ** 3          # some below the albedo floor
    ac = np.concatenate([alb, np.ones((H, W, 1), np.float32)], -1).astype(np.float32)
    return ac, np.concatenate([n, z], -1).astype(np.float32)


def test_denoise_equals_restatement_on_random_features_8_iterations(mcpt, oracle_mod):
    rng = np.random.default_rng(11)
    H, W = 13, 19
    ac, nd = _random_features(rng, H, W)
    # smooth the features a little so that non-centre weights are not all zero
    nd[..., :3] = R.normalize_cu((nd[..., :3] + np.float32(3) * np.array([0, 0, 1], np.float32)).astype(np.float32))
    color = rng.random((H, W, 3)).astype(np.float32)
    kw = dict(iterations=8, normal_power_log2=2, sigma_z=0.5, albedo_floor=0.05)
    got = mcpt.denoise(color, ac, nd, **kw)
    _assert_equal(got, R.denoise(oracle_mod, color, ac, nd, **kw), "denoise x8")
    assert np.abs(got - color).max() > 1e-3


@pytest.mark.parametrize("H,W", [(1, 1), (1, 17), (17, 1), (16, 16), (17, 33)], ids=lambda v: str(v))
def test_denoise_at_degenerate_sizes(mcpt, oracle_mod, H, W):
    """one pixel, one row, one column, one 16x16 workgroup, one more than two: at 5 iterations the
    steps of 8 and 16 reach past every such frame (at 1x1 only the centre tap is left)"""
    rng = np.random.default_rng(100 * H + W)
    ac, nd = _random_features(rng, H, W)
    nd[..., :3] = R.normalize_cu((nd[..., :3] + np.float32(3) * np.array([0, 0, 1], np.float32)).astype(np.float32))
    color = rng.random((H, W, 3)).astype(np.float32)
    kw = dict(iterations=5, normal_power_log2=2, sigma_z=0.5)
    got = mcpt.denoise(color, ac, nd, **kw)
    assert got.shape == (H, W, 3) and np.isfinite(got).all()
    _assert_equal(got, R.denoise(oracle_mod, color, ac, nd, **kw), f"denoise {W}x{H}")
    if H * W > 1:
        assert np.abs(got - color).max() > 1e-3


def test_denoise_gamma_space(mcpt, oracle_mod, real_features):
    H, W = 20, 24
    ac, nd = (np.ascontiguousarray(a[:H, :W]) for a in real_features)
    color = np.random.default_rng(3).random((H, W, 3)).astype(np.float32)
    got = mcpt.denoise(color, ac, nd, gamma_space=True)
    _assert_equal(got, R.denoise(oracle_mod, color, ac, nd, gamma_space=True), "gamma")
    assert not np.array_equal(got, mcpt.denoise(color, ac, nd))


def test_denoise_host_and_device_entries_agree_and_repeat(mcpt, real_features):
    import torch
    ac, nd = real_features
    H, W = ac.shape[:2]
    color = (np.random.default_rng(8).random((H, W, 3)) * 1.5).astype(np.float32)
    host = mcpt.denoise(color, ac, nd, iterations=4)
    rgba = np.concatenate([color, np.full((H, W, 1), 7.0, np.float32)], -1)     # alpha is ignored
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rgba, ac, nd)]
    outs = []
    for _ in range(2):
        out = torch.full((H, W, 4), -1.0, device="cuda")
        scratch = torch.full((H, W, 4), -1.0, device="cuda")
        mcpt.denoise_device(W, H, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(),
                            scratch.data_ptr(), iterations=4)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(t[0].cpu().numpy(), rgba)                              # the input colour is only read
    _assert_equal(outs[0], outs[1], "two runs")
    _assert_equal(outs[0][..., :3], host, "device vs host")
    assert (outs[0][..., 3] == 0).all()                                          # output alpha 0
    with pytest.raises(mcpt.McptError):                                          # out aliasing an input
        mcpt.denoise_device(W, H, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[0].data_ptr(),
                            t[1].data_ptr())


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_render_aov_denoise_lowers_the_error(mcpt, oracle_mod):
    """The public pipeline at 4 spp against a converged 1024-spp render of other samples."""
    scene, _, _ = _scene(mcpt, oracle_mod, "scene01")
    W, H = 64, 48
    ref, _ = scene.render(mcpt.RenderParams(width=W, height=H, spp=1024, spp_offset=100000))
    noisy, _ = scene.render(mcpt.RenderParams(width=W, height=H, spp=4))
    ac, nd = scene.render_aov(mcpt.RenderParams(width=W, height=H, spp=4))
    den = mcpt.denoise(noisy, ac, nd)
    e_noisy, e_den = _rmse(noisy, ref), _rmse(den, ref)
    print(f"RMSE noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
    assert np.isfinite(den).all()
    assert e_den < e_noisy


def test_no_side_effects_on_renders_stats_and_memory(mcpt, oracle_mod):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    p = mcpt.RenderParams(width=48, height=32, spp=4, spp_chunk=2)
    ac = torch.zeros((p.height, p.width, 4), device="cuda")
    nd = torch.zeros_like(ac)
    out = torch.zeros_like(ac)
    scratch = torch.zeros_like(ac)
    torch.cuda.synchronize()
    scene.reserve(p)
    free0 = scene.plan(p)["device_free_bytes"]
    scene.render_aov_device(p, ac.data_ptr(), nd.data_ptr())       # after a reserve: no allocation
    torch.cuda.synchronize()
    assert scene.plan(p)["device_free_bytes"] == free0
    scene.stats()                                                   # a fresh record
    before, st0 = scene.render(p)
    for _ in range(2):
        scene.render_aov_device(p, ac.data_ptr(), nd.data_ptr())
        mcpt.denoise_device(p.width, p.height, ac.data_ptr(), ac.data_ptr(), nd.data_ptr(), out.data_ptr(),
                            scratch.data_ptr())
    torch.cuda.synchronize()
    scene.render_aov(p)
    pending = scene.stats()
    assert pending["renders"] == 0 and pending["rays"] == 0        # feature calls are not renders
    after, st1 = scene.render(p)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert st0["renders"] == st1["renders"] == 1 and st0["rays"] == st1["rays"]
    assert float(ac[..., 3].mean()) > 0.5
