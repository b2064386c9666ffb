"""The temporal-accumulation kernel (csrc/temporal.hip) against the closed-form reprojection of
tests/_temporal_closed.py: the cases tests/test_temporal_closed_cpu.py runs on the numpy
restatement, here on `mcpt.temporal` (one of them through `temporal_device` as well), and the
GPU's own 64-spp feature buffers against the reference's pixel-centre rays cast through
`Scene.intersect`.  Colours, history lengths, variances and coordinates are the kernel's; the
per-pixel class and tap counts next to them are the restatement's on the same inputs.
"""
import numpy as np
import pytest

import _temporal_cases as K
import _temporal_closed as X
import _temporal_ref as T

pytestmark = pytest.mark.gpu

f32 = np.float32
ARGS = ("color", "var", "albedo_cov", "normal_depth", "hist_color_n", "hist_var", "hist_albedo_cov", "hist_normal_depth")


def _render_params(mcpt, mode, W, H, cam, **kw):
    cam = dict(cam)
    if "fov" in cam:
        cam["fov_deg"] = cam.pop("fov")
    if mode == "qe":
        return mcpt.RenderParams.for_quinengine(width=W, height=H, seed=K.QE_SEED, **cam, **kw)
    return mcpt.RenderParams(width=W, height=H, **cam, **kw)


def _classes(oracle_mod, mode, W, H, cur_kw, prev_kw, bufs, params):
    _, _, cls, (offered, used) = T.temporal(
        oracle_mod, T.camera(oracle_mod, W, H, mode, **cur_kw), T.camera(oracle_mod, W, H, mode, **prev_kw),
        mode=mode, return_taps=True, **bufs, **params)
    return cls, offered, used


@pytest.fixture(scope="module")
def run(mcpt, oracle_mod):
    def go(mode, W, H, cur_kw, prev_kw, bufs, **params):
        out, out_var = mcpt.temporal(_render_params(mcpt, mode, W, H, cur_kw), _render_params(mcpt, mode, W, H, prev_kw),
                                     *[bufs[a] for a in ARGS], **params)
        return X.Result(out, out_var, *_classes(oracle_mod, mode, W, H, cur_kw, prev_kw, bufs, params))
    return go


@pytest.fixture(scope="module")
def run_device(mcpt, oracle_mod):
    import torch

    def go(mode, W, H, cur_kw, prev_kw, bufs, **params):
        rgba = np.concatenate([bufs["color"], np.full((H, W, 1), 7.0, f32)], -1)   # the colour's alpha is ignored
        host = [rgba if a == "color" else bufs[a] for a in ARGS]
        dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, f32)).cuda() for a in host]
        out = torch.full((H, W, 4), -1.0, device="cuda")
        out_var = None if bufs["var"] is None else torch.full((H, W, 4), -1.0, device="cuda")
        mcpt.temporal_device(_render_params(mcpt, mode, W, H, cur_kw), _render_params(mcpt, mode, W, H, prev_kw),
                             *[0 if t is None else t.data_ptr() for t in dev], out.data_ptr(),
                             0 if out_var is None else out_var.data_ptr(), **params)
        torch.cuda.synchronize()
        return X.Result(out.cpu().numpy(), None if out_var is None else out_var.cpu().numpy(),
                        *_classes(oracle_mod, mode, W, H, cur_kw, prev_kw, bufs, params))
    return go


@pytest.mark.parametrize("pair", ["all", "dolly", "long"])
@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", X.MODES)
def test_reprojection_lands_where_the_projection_says(run, mode, size, pair):
    X.check_reprojection(run, mode, *size, *X.pairs(mode)[pair])


@pytest.mark.parametrize("mode", X.MODES)
def test_the_device_entry_lands_there_too(run_device, mode):
    X.check_reprojection(run_device, mode, 37, 23, *X.pairs(mode)["all"])
    X.check_variance(run_device, mode, 37, 23)


@pytest.mark.parametrize("mode", X.MODES)
def test_the_depth_term_two_sided(run, mode):
    X.check_depth_term(run, mode)


@pytest.mark.parametrize("thr", [0.9, 0.5])
@pytest.mark.parametrize("mode", X.MODES)
def test_the_normal_test_scales_with_both_coverages(run, mode, thr):
    X.check_normal_test(run, mode, thr)


@pytest.mark.parametrize("world", sorted(X.disocclusion_worlds()))
@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", X.MODES)
def test_history_never_crosses_a_silhouette(run, mode, size, world):
    X.check_disocclusion(run, mode, *size, world)


@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", X.MODES)
def test_variance_of_full_and_rim_footprints(run, mode, size):
    X.check_variance(run, mode, *size)


@pytest.mark.parametrize("mode", X.MODES)
def test_six_frames_follow_the_recurrence(run, mode):
    X.check_blend(run, mode)


@pytest.mark.parametrize("mode", X.MODES)
def test_gamma_space_decodes_this_frame_only(run, mode):
    X.check_gamma(run, mode)


@pytest.mark.parametrize("cam", sorted(X.RENDER_CAMERAS))
@pytest.mark.parametrize("mode", X.MODES)
def test_the_renders_mean_depth_is_the_centre_rays(mcpt, mode, cam):
    W, H = K.W0, K.H0
    cam_kw = X.RENDER_CAMERAS[cam]
    name, flavor = ("qe_scene01", "tinyobj") if mode == "qe" else ("scene01", "cvmctracer")
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name), flavor=flavor))
    ac, nd = scene.render_aov(_render_params(mcpt, mode, W, H, cam_kw, spp=X.RENDER_SPP))
    o, d = X.centre_rays(mode, W, H, cam_kw)
    tri, hit, _ = scene.intersect(o, d)
    X.check_centre_fit(ac, nd, hit[:, 2].reshape(H, W), (tri >= 0).reshape(H, W), f"{mode} {cam}")
