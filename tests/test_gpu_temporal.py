"""Temporal accumulation (csrc/temporal.hip) on the GPU, bit for bit against its numpy
restatement (tests/_temporal_ref.py): scene01 frames under the camera pairs of
tests/_temporal_cases.py (the GPU's own 4-spp feature buffers and 8-spp render_var frames),
QuinEngine mode with a gamma-encoded framebuffer, another aspect and field of view, synthetic
frames at degenerate sizes with NaN and infinities in the rejected history, the entry forms,
a ping-pong into the variance-guided denoiser, and one check of what accumulation is for.
"""
import numpy as np
import pytest

import _temporal_cases as K
import _temporal_ref as T

pytestmark = pytest.mark.gpu

f32 = np.float32
_scenes, _frames = {}, {}


def _scene(mcpt, mode="cv"):
    if mode not in _scenes:
        name, flavor = ("qe_scene01", "tinyobj") if mode == "qe" else ("scene01", "cvmctracer")
        _scenes[mode] = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name), flavor=flavor))
    return _scenes[mode]


def _render_params(mcpt, mode, W, H, cam, **kw):
    cam = dict(cam)
    if "fov" in cam:
        cam["fov_deg"] = cam.pop("fov")
    if mode == "qe":
        return mcpt.RenderParams.for_quinengine(width=W, height=H, seed=K.QE_SEED, **cam, **kw)
    return mcpt.RenderParams(width=W, height=H, **cam, **kw)


def _frame(mcpt, mode, W, H, cam, spp=8, chunk=4, spp_offset=0):
    """(fb (H, W, 3), var, albedo_cov, normal_depth) of one camera on the GPU, rendered once"""
    key = (mode, W, H, spp, chunk, spp_offset, tuple(sorted((k, v) for k, v in cam.items())))
    if key not in _frames:
        scene = _scene(mcpt, mode)
        fb, var, _ = scene.render_var(_render_params(mcpt, mode, W, H, cam, spp=spp, spp_chunk=chunk,
                                                     spp_offset=spp_offset))
        ac, nd = scene.render_aov(_render_params(mcpt, mode, W, H, cam, spp=K.FEATURE_SPP))
        _frames[key] = (fb, var, ac, nd)
    return _frames[key]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _assert_equal(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(),
                           np.asarray(got)[bad][:5].tolist(), np.asarray(ref)[bad][:5].tolist())


def _counts(cls):
    return {T.CLASS_NAMES[k]: int((cls == k).sum()) for k in range(5)}


def _history(mode, prev_frame):
    """the previous frame as a history: its colour (linear), the fixed pattern of lengths, its variance"""
    fb, var = prev_frame[0], prev_frame[1]
    lin = np.power(fb, f32(2.2)).astype(f32) if mode == "qe" else fb
    H, W = fb.shape[:2]
    return np.concatenate([lin, K.history_lengths(H, W)[..., None]], -1).astype(f32), var


@pytest.mark.parametrize("case", sorted(K.SCENE_CASES))
def test_scene_frames_equal_the_restatement(mcpt, oracle_mod, case):
    mode, W, H, cur, prev, named = K.SCENE_CASES[case]
    fb, var, ac, nd = _frame(mcpt, mode, W, H, cur)
    pf = _frame(mcpt, mode, W, H, prev)
    hcol, hvar = _history(mode, pf)
    kw = dict(gamma_space=True) if mode == "qe" else {}
    got, got_var = mcpt.temporal(_render_params(mcpt, mode, W, H, cur), _render_params(mcpt, mode, W, H, prev),
                                 fb, var, ac, nd, hcol, hvar, pf[2], pf[3], **kw)
    ref, ref_var, cls = T.temporal(oracle_mod, T.camera(oracle_mod, W, H, mode, **cur),
                                   T.camera(oracle_mod, W, H, mode, **prev), fb, var, ac, nd, hcol, hvar, pf[2], pf[3],
                                   mode=mode, **kw)
    print(case, _counts(cls))
    assert set(named) <= K.populated(cls), (case, _counts(cls))
    assert got.shape == (H, W, 4) and got_var.shape == (H, W, 4) and np.isfinite(got).all()
    _assert_equal(got, ref, f"{case}: colour and N")
    _assert_equal(got_var, ref_var, f"{case}: variance")
    reset = np.isin(cls, (T.MISS, T.BEHIND, T.REJECTED))
    assert (got[..., 3][reset] == 1).all() and (got[..., 3][~reset] > 1).all() and got[..., 3].max() <= 32
    assert (got_var[..., 3] == 0).all()
    if case == "turn120":
        _assert_equal(got[..., :3], fb, "every pixel reset: the frame itself")
        _assert_equal(got_var, var, "every pixel reset: its variance")
    else:
        assert not np.array_equal(got[..., :3], fb)


@pytest.mark.parametrize("kw", [dict(max_history=1), dict(max_history=5, normal_threshold=0.5, sigma_z=0.02),
                                dict(max_history=65536, normal_threshold=1.0, sigma_z=1.5)],
                         ids=["no-accumulation", "tight-depth", "loose-depth"])
def test_parameters_reach_the_kernel(mcpt, oracle_mod, kw):
    mode, W, H, cur, prev, _ = K.SCENE_CASES["yaw2"]
    fb, var, ac, nd = _frame(mcpt, mode, W, H, cur)
    pf = _frame(mcpt, mode, W, H, prev)
    hcol, hvar = _history(mode, pf)
    got, got_var = mcpt.temporal(_render_params(mcpt, mode, W, H, cur), _render_params(mcpt, mode, W, H, prev),
                                 fb, var, ac, nd, hcol, hvar, pf[2], pf[3], **kw)
    ref, ref_var, cls = T.temporal(oracle_mod, T.camera(oracle_mod, W, H, mode, **cur),
                                   T.camera(oracle_mod, W, H, mode, **prev), fb, var, ac, nd, hcol, hvar, pf[2], pf[3],
                                   mode=mode, **kw)
    print(kw, _counts(cls))
    _assert_equal(got, ref, "colour and N")
    _assert_equal(got_var, ref_var, "variance")
    assert got[..., 3].max() <= kw["max_history"]
    if kw["max_history"] == 1:
        assert np.array_equal(got[..., :3], fb) and (got[..., 3] == 1).all() and np.array_equal(got_var, var)
    else:
        assert (cls == T.BILINEAR).any()


@pytest.mark.parametrize("size", K.SYNTHETIC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_frames_at_degenerate_sizes(mcpt, oracle_mod, size):
    """one pixel, one column, one 16 x 16 workgroup, 3 x 5 of them partly filled; what a rejected
    history pixel holds (NaN, +-inf) never reaches an output"""
    W, H = size
    (cur, cur_kw), (prev, prev_kw), bufs = K.synthetic(oracle_mod, W, H, K.synthetic_seed(W, H))
    ref, ref_var, cls, (offered, used) = T.temporal(oracle_mod, cur, prev, **bufs, return_taps=True)
    partial = (cls == T.BILINEAR) & (used < offered)
    print(size, _counts(cls), "partly valid", int(partial.sum()))
    if W * H >= 256:
        assert (cls == T.FALLBACK).sum() >= W * H // 8 and partial.sum() >= W * H // 8
        assert not np.isfinite(bufs["hist_color_n"]).all() and not np.isfinite(bufs["hist_var"]).all()
    got, got_var = mcpt.temporal(_render_params(mcpt, "cv", W, H, cur_kw), _render_params(mcpt, "cv", W, H, prev_kw),
                                 bufs["color"], bufs["var"], bufs["albedo_cov"], bufs["normal_depth"],
                                 bufs["hist_color_n"], bufs["hist_var"], bufs["hist_albedo_cov"],
                                 bufs["hist_normal_depth"])
    assert np.isfinite(got).all() and np.isfinite(got_var).all()
    _assert_equal(got, ref, f"{W}x{H}: colour and N")
    _assert_equal(got_var, ref_var, f"{W}x{H}: variance")


def test_without_variance_the_colour_is_the_same(mcpt):
    mode, W, H, cur, prev, _ = K.SCENE_CASES["shift"]
    fb, var, ac, nd = _frame(mcpt, mode, W, H, cur)
    pf = _frame(mcpt, mode, W, H, prev)
    hcol, hvar = _history(mode, pf)
    pc, pp = _render_params(mcpt, mode, W, H, cur), _render_params(mcpt, mode, W, H, prev)
    with_var, v = mcpt.temporal(pc, pp, fb, var, ac, nd, hcol, hvar, pf[2], pf[3])
    without, none = mcpt.temporal(pc, pp, fb, None, ac, nd, hcol, None, pf[2], pf[3])
    assert none is None and v is not None
    _assert_equal(without, with_var, "colour without variance")


def test_host_and_device_entries_agree_and_repeat(mcpt):
    import torch
    mode, W, H, cur, prev, _ = K.SCENE_CASES["yaw2"]
    fb, var, ac, nd = _frame(mcpt, mode, W, H, cur)
    pf = _frame(mcpt, mode, W, H, prev)
    hcol, hvar = _history(mode, pf)
    pc, pp = _render_params(mcpt, mode, W, H, cur), _render_params(mcpt, mode, W, H, prev)
    host, host_var = mcpt.temporal(pc, pp, fb, var, ac, nd, hcol, hvar, pf[2], pf[3])
    rgba = np.concatenate([fb, np.full((H, W, 1), 7.0, f32)], -1)          # the colour's alpha is ignored
    ins = [rgba, var, ac, nd, hcol, hvar, pf[2], pf[3]]
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins]
    ptrs = [x.data_ptr() for x in t]
    outs = []
    for _ in range(2):
        out = torch.full((H, W, 4), -1.0, device="cuda")
        out_var = torch.full((H, W, 4), -1.0, device="cuda")
        mcpt.temporal_device(pc, pp, *ptrs, out.data_ptr(), out_var.data_ptr())
        torch.cuda.synchronize()
        outs.append((out.cpu().numpy(), out_var.cpu().numpy()))
    for a, x in zip(ins, t):
        assert np.array_equal(x.cpu().numpy(), a)                          # inputs only read
    _assert_equal(outs[0][0], outs[1][0], "two runs: colour")
    _assert_equal(outs[0][1], outs[1][1], "two runs: variance")
    _assert_equal(outs[0][0], host, "device vs host: colour")
    _assert_equal(outs[0][1], host_var, "device vs host: variance")
    # on a side stream, without variance: the same colour
    st = torch.cuda.Stream()
    out = torch.full((H, W, 4), -1.0, device="cuda")
    torch.cuda.synchronize()
    mcpt.temporal_device(pc, pp, ptrs[0], 0, ptrs[2], ptrs[3], ptrs[4], 0, ptrs[6], ptrs[7], out.data_ptr(), 0,
                         stream_ptr=st.cuda_stream)
    st.synchronize()
    _assert_equal(out.cpu().numpy(), host, "side stream, no variance")
    with pytest.raises(mcpt.McptError) as e:                               # an output aliasing an input
        mcpt.temporal_device(pc, pp, *ptrs, ptrs[4], out.data_ptr())
    assert "overlap" in str(e.value)


def test_three_frame_ping_pong_feeds_the_variance_guided_denoiser(mcpt):
    W, H = K.W0, K.H0
    hist = None
    for i, deg in enumerate((0.0, 1.5, 3.0)):
        cam = dict(eye=(0.2 * i, 5.0, 17.0), direction=K.yaw(deg))
        fb, var, ac, nd = _frame(mcpt, "cv", W, H, cam, spp=2, chunk=1, spp_offset=2 * i)
        if hist is None:
            col = np.concatenate([fb, np.ones((H, W, 1), f32)], -1).astype(f32)
            cvar = var
        else:
            col, cvar = mcpt.temporal(_render_params(mcpt, "cv", W, H, cam), _render_params(mcpt, "cv", W, H, hist[0]),
                                      fb, var, ac, nd, hist[1], hist[2], hist[3], hist[4], max_history=2)
            assert col[..., 3].max() == 2 and col[..., 3].min() == 1       # never past max_history
            assert (col[..., 3] == 2).mean() > 0.5
        hist = (cam, col, cvar, ac, nd)
    den = mcpt.denoise_var(np.ascontiguousarray(col[..., :3]), cvar, ac, nd)
    assert den.shape == (H, W, 3) and np.isfinite(den).all() and not np.array_equal(den, col[..., :3])
    assert np.isfinite(cvar).all() and (cvar >= 0).all() and (cvar[..., 3] == 0).all()


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_accumulating_over_a_moving_camera_beats_the_last_frame_alone(mcpt):
    """8 frames at 2 spp of a camera yawing half a degree per frame, against a 4096-spp render of
    other samples from the last camera: an inequality, no threshold."""
    W, H = 64, 48
    scene = _scene(mcpt)
    hist = None
    for i in range(8):
        cam = dict(eye=(0.0, 5.0, 17.0), direction=K.yaw(0.5 * i))
        fb, var, ac, nd = _frame(mcpt, "cv", W, H, cam, spp=2, chunk=1, spp_offset=2 * i)
        if hist is None:
            col, cvar = np.concatenate([fb, np.ones((H, W, 1), f32)], -1).astype(f32), var
        else:
            col, cvar = mcpt.temporal(_render_params(mcpt, "cv", W, H, cam), _render_params(mcpt, "cv", W, H, hist[0]),
                                      fb, var, ac, nd, hist[1], hist[2], hist[3], hist[4])
        hist = (cam, col, cvar, ac, nd)
    ref, _ = scene.render(_render_params(mcpt, "cv", W, H, cam, spp=4096, spp_offset=100000))
    last, accumulated = _rmse(fb, ref), _rmse(col[..., :3], ref)
    print(f"RMSE last frame {last:.4f} accumulated {accumulated:.4f}; N mean {col[..., 3].mean():.2f}")
    assert 7.5 < col[..., 3].max() < 8.5                                   # (N is interpolated: not an integer)
    assert accumulated < last
