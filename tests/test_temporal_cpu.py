"""Temporal accumulation (csrc/temporal.hip) without a GPU: the entries
and their defaults, every argument check of mcpt_temporal / mcpt_temporal_device with its code,
in the header's order and before any device call (the pointers are fakes: a call that got past
the checks would fault), and the properties of the numpy restatement (tests/_temporal_ref.py)
on the oracle's feature buffers of scene01 at 37 x 23, 4 spp -- among them that every frame
pair tests/test_gpu_temporal.py compares on the GPU populates the classes it names.

Equal cameras, measured: at the default camera 580 of the 731 covered pixels (79.3%) are class
bilinear.  The other 151 are pixels whose own 4-sample mean normal is too short for the normal
test against itself (|n|^2 < 0.9 cov^2): with +-1 pixel of jitter a fifth of this small frame's
pixels average the normals of two surfaces.  That is the specified test, not a reprojection
error -- test_equal_cameras_at_the_default_camera pins exactly that -- so the 90% property is
asserted from a camera with fewer such pixels (eye z = 12, fov 30: 836 of 851, 98.2%).
"""
import ctypes as C

import numpy as np
import pytest

import _aov_ref as A
import _temporal_cases as K
import _temporal_ref as T

f32 = np.float32
INVALID, UNSUPPORTED = -1, -6


# ---- the entries and their checks -------------------------------------------------------------

def _capi():
    from montecarlopathtracer_amd import _capi
    return _capi


def test_entries_exist_and_the_defaults_are_spelled_out(mcpt):
    capi = _capi()
    L = capi.lib()
    for name in ("mcpt_temporal_params_default", "mcpt_temporal", "mcpt_temporal_device"):
        assert hasattr(L, name), name
    t = capi.TemporalParamsC(-5, -5.0, -5.0, -5)
    L.mcpt_temporal_params_default(C.byref(t))
    assert (t.max_history, t.normal_threshold, t.sigma_z, t.gamma_space) == (32, float(f32(0.9)), float(f32(0.1)), 0)
    L.mcpt_temporal_params_default(None)                     # a NULL struct is ignored
    assert L.mcpt_abi_version() == 9
    z = mcpt.temporal_params()
    assert (z.max_history, z.normal_threshold, z.sigma_z, z.gamma_space) == (0, 0.0, 0.0, 0)   # 0 = the default
    for f in ("temporal", "temporal_device", "temporal_params"):
        assert f in mcpt.__all__ and callable(getattr(mcpt, f))


NAMES = ("color", "var", "albedo_cov", "normal_depth", "hist_color_n", "hist_var", "hist_albedo_cov",
         "hist_normal_depth", "out_color_n", "out_var")
VAR_NAMES = ("var", "hist_var", "out_var")


def _fake_ptrs(W, H):
    """ten addresses no two of whose W x H x 16-byte ranges overlap (never dereferenced)"""
    stride = ((W * H * 16 + 0xFFFF) // 0x10000 + 1) * 0x10000
    return {n: 0x10000 + i * stride for i, n in enumerate(NAMES)}


def _call(mcpt, entry, tp, cur, prev, ptrs):
    """mcpt_temporal / mcpt_temporal_device on fake pointers: (code, message)"""
    capi = _capi()
    L = capi.lib()
    ref = lambda s: None if s is None else C.byref(s)   # noqa: E731
    if entry == "device":
        args = [C.c_void_p(ptrs[n] or None) for n in NAMES] + [C.c_void_p(None)]
        rc = L.mcpt_temporal_device(ref(tp), ref(cur), ref(prev), *args)
    else:
        args = [C.cast(C.c_void_p(ptrs[n] or None), C.POINTER(C.c_float)) for n in NAMES]
        rc = L.mcpt_temporal(ref(tp), ref(cur), ref(prev), *args)
    return rc, L.mcpt_last_error().decode()


def _params(mcpt, W=8, H=8, mode=0):
    p = mcpt.RenderParams(width=W, height=H).to_c()
    p.mode = mode
    return p


ENTRIES = ["device", "host"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_check_1_a_null_required_pointer_comes_first(mcpt, entry):
    bad_tp = mcpt.temporal_params(max_history=-1)            # (check 2 would fire too)
    for missing in ("cur", "prev") + tuple(n for n in NAMES if n not in VAR_NAMES):
        cur, prev, ptrs = _params(mcpt, 0, 0), _params(mcpt, 0, 0), _fake_ptrs(8, 8)   # (and check 3)
        if missing == "cur":
            cur = None
        elif missing == "prev":
            prev = None
        else:
            ptrs[missing] = 0
        rc, msg = _call(mcpt, entry, bad_tp, cur, prev, ptrs)
        assert rc == INVALID and "NULL" in msg, (missing, rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_check_2_a_params_field_out_of_range_is_named(mcpt, entry):
    bad = [("max_history", dict(max_history=-1)), ("max_history", dict(max_history=65537)),
           ("normal_threshold", dict(normal_threshold=-0.5)), ("normal_threshold", dict(normal_threshold=1.5)),
           ("normal_threshold", dict(normal_threshold=float("nan"))),
           ("sigma_z", dict(sigma_z=-1.0)), ("sigma_z", dict(sigma_z=float("inf"))),
           ("sigma_z", dict(sigma_z=float("nan")))]
    for field, kw in bad:
        rc, msg = _call(mcpt, entry, mcpt.temporal_params(**kw), _params(mcpt, 0, 8), _params(mcpt, 0, 8),
                        _fake_ptrs(8, 8))                    # (width 0: check 3 would fire too)
        assert rc == INVALID and field in msg, (kw, rc, msg)
    tp = mcpt.temporal_params()
    tp.gamma_space = 2
    rc, msg = _call(mcpt, entry, tp, _params(mcpt, 0, 8), _params(mcpt, 0, 8), _fake_ptrs(8, 8))
    assert rc == INVALID and "gamma_space" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_checks_3_to_5_sizes_modes_and_the_two_cameras(mcpt, entry):
    tp, ptrs = mcpt.temporal_params(), _fake_ptrs(8, 8)
    for W, H in ((0, 8), (8, 0), (-3, 8)):                   # 3 before 4: the mode is unknown as well
        rc, msg = _call(mcpt, entry, tp, _params(mcpt, W, H, mode=7), _params(mcpt, W, H, mode=7), ptrs)
        assert rc == INVALID and "width/height" in msg, (W, H, rc, msg)
    # 4 before 5: prev differs in every field
    rc, msg = _call(mcpt, entry, tp, _params(mcpt, 8, 8, mode=7), _params(mcpt, 9, 9, mode=0), ptrs)
    assert rc == INVALID and "unknown mode" in msg, (rc, msg)
    partial = dict(ptrs, hist_var=0)                         # 5 before 6: the variance pointers are partial
    for field, prev in (("width", _params(mcpt, 9, 8)), ("height", _params(mcpt, 8, 9)),
                        ("mode", _params(mcpt, 8, 8, mode=1))):
        rc, msg = _call(mcpt, entry, tp, _params(mcpt, 8, 8), prev, partial)
        assert rc == INVALID and field in msg and "differ" in msg, (field, rc, msg)
    rc, msg = _call(mcpt, entry, None, _params(mcpt, 8, 8), _params(mcpt, 9, 8), ptrs)   # tp NULL: the defaults
    assert rc == INVALID and "width" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_checks_6_to_8_variance_pointers_size_and_overlap(mcpt, entry):
    tp = mcpt.temporal_params()
    big = 32768                                              # 2^30 pixels: past 2^31 / 3 (check 7 would fire too)
    for given in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        ptrs = _fake_ptrs(8, 8)
        for n, g in zip(VAR_NAMES, given):
            if not g:
                ptrs[n] = 0
        rc, msg = _call(mcpt, entry, tp, _params(mcpt, big, big), _params(mcpt, big, big), ptrs)
        assert rc == INVALID and "together" in msg, (given, rc, msg)
    # 7 before 8: every pointer the same
    same = {n: 0x10000 for n in NAMES}
    rc, msg = _call(mcpt, entry, tp, _params(mcpt, big, big), _params(mcpt, big, big), same)
    assert rc == UNSUPPORTED and "2^31 / 3" in msg, (rc, msg)
    limit = (1 << 31) // 3                                   # the first pixel count refused ...
    rc, msg = _call(mcpt, entry, tp, _params(mcpt, limit, 1), _params(mcpt, limit, 1), same)
    assert rc == UNSUPPORTED, (rc, msg)
    rc, msg = _call(mcpt, entry, tp, _params(mcpt, limit - 1, 1), _params(mcpt, limit - 1, 1), same)
    assert rc == INVALID and "overlap" in msg, (rc, msg)    # ... and the last one let through to check 8
    # 8: either output against every input and against the other output, partial overlaps too
    W = H = 8
    size = W * H * 16
    for out in ("out_color_n", "out_var"):
        for other in NAMES:
            if other == out:
                continue
            for off in (0, 16, size - 16, -(size - 16)):
                ptrs = _fake_ptrs(W, H)
                ptrs[out] = ptrs[other] + off
                rc, msg = _call(mcpt, entry, tp, _params(mcpt, W, H), _params(mcpt, W, H), ptrs)
                assert rc == INVALID and "overlap" in msg, (out, other, off, rc, msg)
    ptrs = _fake_ptrs(W, H)                                  # without variance: the colour output alone
    for n in VAR_NAMES:
        ptrs[n] = 0
    ptrs["out_color_n"] = ptrs["hist_normal_depth"] + 16
    rc, msg = _call(mcpt, entry, tp, _params(mcpt, W, H), _params(mcpt, W, H), ptrs)
    assert rc == INVALID and "overlap" in msg, (rc, msg)


def test_python_mirror_rejects_before_it_calls(mcpt):
    a = np.zeros((4, 4, 4), f32)
    p = mcpt.RenderParams(width=4, height=4)
    with pytest.raises(mcpt.McptError):
        mcpt.temporal(p, p, np.zeros((4, 4, 2), f32), a, a, a, a, a, a, a)
    with pytest.raises(mcpt.McptError):
        mcpt.temporal(p, p, a, a, a, a, a, None, a, a)       # variance without hist_var
    with pytest.raises(mcpt.McptError):
        mcpt.temporal(p, p, a, a, a, np.zeros((4, 3, 4), f32), a, a, a, a)
    with pytest.raises(mcpt.McptError) as e:                 # the library's own check, through the mirror
        mcpt.temporal(p, mcpt.RenderParams(width=4, height=5), a, a, a, a, a, a, a, a)
    assert e.value.code == INVALID and "height" in str(e.value)


# ---- the restatement's properties on oracle-made feature buffers --------------------------------

_o_scenes, _features = {}, {}


def _o_scene(oracle_mod, mcpt, mode):
    if mode not in _o_scenes:
        _o_scenes[mode] = (oracle_mod.Scene(mcpt.scene_path("qe_scene01"), flavor="tinyobj") if mode == "qe"
                           else oracle_mod.Scene(mcpt.scene_path("scene01")))
    return _o_scenes[mode]


def _feat(oracle_mod, mcpt, mode, W, H, cam):
    """the oracle's (albedo_cov, normal_depth) of one frame, computed once"""
    key = (mode, W, H, tuple(sorted((k, tuple(v) if isinstance(v, tuple) else v) for k, v in cam.items())))
    if key not in _features:
        kw = dict(seed=K.QE_SEED, fresnel_kd=False) if mode == "qe" else {}
        _features[key] = A.aov_reference(oracle_mod, _o_scene(oracle_mod, mcpt, mode), W, H, K.FEATURE_SPP, mode=mode,
                                         **kw, **cam)
    return _features[key]


def _random_frame(seed, H, W):
    rng = np.random.default_rng(seed)
    color = rng.random((H, W, 3)).astype(f32)
    var = np.concatenate([rng.random((H, W, 3)) * 0.05, np.zeros((H, W, 1))], -1).astype(f32)
    hcol = np.concatenate([rng.random((H, W, 3)).astype(f32), K.history_lengths(H, W)[..., None]], -1).astype(f32)
    hvar = np.concatenate([rng.random((H, W, 3)) * 0.05, np.zeros((H, W, 1))], -1).astype(f32)
    return color, var, hcol, hvar


def _run(oracle_mod, mcpt, mode, W, H, cur, prev, seed=5, **kw):
    ac, nd = _feat(oracle_mod, mcpt, mode, W, H, cur)
    hac, hnd = _feat(oracle_mod, mcpt, mode, W, H, prev)
    color, var, hcol, hvar = _random_frame(seed, H, W)
    out = T.temporal(oracle_mod, T.camera(oracle_mod, W, H, mode, **cur), T.camera(oracle_mod, W, H, mode, **prev),
                     color, var, ac, nd, hcol, hvar, hac, hnd, mode=mode, **kw)
    return (color, var, hcol, hvar, ac, nd), out


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _counts(cls):
    return {T.CLASS_NAMES[k]: int((cls == k).sum()) for k in range(5)}


CLOSE = dict(eye=(0.0, 5.0, 12.0), direction=(0.0, 0.0, -1.0), fov=30.0)


def test_equal_cameras_keep_the_history_of_their_own_pixel(mcpt, oracle_mod):
    W, H = K.W0, K.H0
    (color, var, hcol, hvar, ac, nd), (out, out_var, cls, (offered, used)) = _run(
        oracle_mod, mcpt, "cv", W, H, CLOSE, CLOSE, return_taps=True)
    covered = ac[..., 3] > 0
    share = (cls[covered] == T.BILINEAR).mean()
    print(_counts(cls), "covered", int(covered.sum()), "bilinear share", share)
    assert covered.sum() > 0.9 * W * H
    assert share >= 0.9
    assert not (cls[covered] == T.BEHIND).any()
    assert (cls[~covered] == T.MISS).all()
    # a pixel that lands on itself exactly gets the running mean of its own history, bit for bit
    hit, front, bx, by, _ = T.reproject(T.camera(oracle_mod, W, H, **CLOSE), T.camera(oracle_mod, W, H, **CLOSE), ac, nd)
    exact = (cls == T.BILINEAR) & (bx == np.floor(bx)) & (by == np.floor(by))
    assert exact.sum() >= 20 and (used[exact] == 1).all()
    ys, xs = np.mgrid[0:H, 0:W]
    assert (bx[exact] == xs[exact]).all() and (by[exact] == ys[exact]).all()
    ne = np.minimum(hcol[..., 3], f32(31))
    n1 = ne + f32(1)
    mean = ((hcol[..., :3] * ne[..., None] + color) / n1[..., None]).astype(f32)
    mvar = (((hvar[..., :3] * ne[..., None]) * ne[..., None] + var[..., :3]) / (n1 * n1)[..., None]).astype(f32)
    assert (_bits(out[..., :3])[exact] == _bits(mean)[exact]).all()
    assert (_bits(out[..., 3])[exact] == _bits(n1)[exact]).all()
    assert (_bits(out_var[..., :3])[exact] == _bits(mvar)[exact]).all() and (out_var[..., 3] == 0).all()
    assert (ne[exact] == 31).any() and (ne[exact] < 31).any()      # the cap bites in some, not in others


def test_equal_cameras_at_the_default_camera(mcpt, oracle_mod):
    """Here the share of bilinear pixels is below 90% (the module's docstring): every covered
    pixel that is not class bilinear fails the normal test against its own mean normal."""
    W, H = K.W0, K.H0
    (_, _, _, _, ac, nd), (_, _, cls) = _run(oracle_mod, mcpt, "cv", W, H, K.DEFAULT, K.DEFAULT)
    covered = ac[..., 3] > 0
    cov = ac[..., 3]
    n2 = (nd[..., 0] * nd[..., 0] + nd[..., 1] * nd[..., 1]) + nd[..., 2] * nd[..., 2]
    self_valid = covered & (n2 >= f32(0.9) * (cov * cov))
    print(_counts(cls), "covered", int(covered.sum()), "self-valid", int(self_valid.sum()),
          "bilinear share", (cls[covered] == T.BILINEAR).mean())
    assert not (cls[covered] == T.BEHIND).any()
    assert (cls[self_valid] == T.BILINEAR).all()
    assert (cls[covered & ~self_valid] != T.BILINEAR).sum() >= 100


def test_max_history_1_returns_the_current_frame(mcpt, oracle_mod):
    for cur, prev in ((K.DEFAULT, K.DEFAULT), (K.SCENE_CASES["yaw2"][3], K.DEFAULT)):
        (color, var, _, _, _, _), (out, out_var, cls) = _run(oracle_mod, mcpt, "cv", K.W0, K.H0, cur, prev,
                                                             max_history=1)
        assert (cls == T.BILINEAR).any()
        assert np.array_equal(out[..., :3], color) and (out[..., 3] == 1).all()
        assert np.array_equal(out_var, var)


def test_sideways_shift_populates_every_class_but_behind(mcpt, oracle_mod):
    mode, W, H, cur, prev, _ = K.SCENE_CASES["shift"]
    (_, _, _, _, ac, nd), (out, _, cls) = _run(oracle_mod, mcpt, mode, W, H, cur, prev)
    print(_counts(cls))
    for k in (T.MISS, T.REJECTED, T.BILINEAR, T.FALLBACK):
        assert (cls == k).any(), T.CLASS_NAMES[k]
    # uncovered wall: pixels of the new frame that are sound themselves, land inside the old frame
    # and find a different depth under all four taps
    hac, hnd = _feat(oracle_mod, mcpt, mode, W, H, prev)
    hit, front, bx, by, e = T.reproject(T.camera(oracle_mod, W, H, **cur), T.camera(oracle_mod, W, H, **prev), ac, nd)
    with np.errstate(all="ignore"):
        zq = hnd[..., 3] / hac[..., 3]
        jx = np.clip(np.floor(np.nan_to_num(bx)), 0, W - 2).astype(int)
        jy = np.clip(np.floor(np.nan_to_num(by)), 0, H - 2).astype(int)
        depth_off = np.ones((H, W), bool)
        for dy in (0, 1):
            for dx in (0, 1):
                z = zq[jy + dy, jx + dx]
                depth_off &= ~(np.abs(e - z) <= f32(0.1) * np.fmax(e, z))
    assert ((cls == T.REJECTED) & depth_off & (bx >= 0) & (bx <= W - 1) & (by >= 0) & (by <= H - 1)).sum() >= 3
    reset = np.isin(cls, (T.MISS, T.BEHIND, T.REJECTED))
    assert (out[..., 3][reset] == 1).all() and (out[..., 3][~reset] >= 2).all()     # out.w == 1 marks a reset


def test_a_previous_camera_turned_away_resets_every_pixel(mcpt, oracle_mod):
    mode, W, H, cur, prev, _ = K.SCENE_CASES["turn120"]
    (color, var, _, _, ac, _), (out, out_var, cls) = _run(oracle_mod, mcpt, mode, W, H, cur, prev)
    covered = ac[..., 3] > 0
    assert (cls[covered] == T.BEHIND).all() and (cls[~covered] == T.MISS).all()
    assert np.array_equal(out[..., :3], color) and (out[..., 3] == 1).all() and np.array_equal(out_var, var)


@pytest.mark.parametrize("case", sorted(K.SCENE_CASES))
def test_every_gpu_frame_pair_populates_the_classes_it_names(mcpt, oracle_mod, case):
    mode, W, H, cur, prev, named = K.SCENE_CASES[case]
    _, (_, _, cls) = _run(oracle_mod, mcpt, mode, W, H, cur, prev)
    print(case, _counts(cls))
    assert set(named) <= K.populated(cls), (case, _counts(cls))


@pytest.mark.parametrize("size", K.SYNTHETIC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_frames_populate_fallback_and_partly_valid_footprints(oracle_mod, size):
    W, H = size
    (cur, _), (prev, _), bufs = K.synthetic(oracle_mod, W, H, K.synthetic_seed(W, H))
    out, out_var, cls, (offered, used) = T.temporal(oracle_mod, cur, prev, **bufs, return_taps=True)
    partial = (cls == T.BILINEAR) & (used < offered)
    print(size, _counts(cls), "partly valid", int(partial.sum()))
    assert np.isfinite(out).all() and np.isfinite(out_var).all()      # no rejected pixel reaches an output
    if W * H >= 256:
        assert not np.isfinite(bufs["hist_color_n"]).all() and not np.isfinite(bufs["hist_var"]).all()
        assert (cls == T.FALLBACK).sum() >= W * H // 8 and partial.sum() >= W * H // 8
        assert (cls == T.REJECTED).any()
    assert K.populated(cls) <= {T.REJECTED, T.BILINEAR, T.FALLBACK}
