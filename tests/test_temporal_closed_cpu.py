"""The numpy restatement of the temporal accumulation (tests/_temporal_ref.py) against the
closed-form reprojection of tests/_temporal_closed.py, without a GPU: the cases
tests/test_gpu_temporal_closed.py runs on the kernel, the reference's own consistency first,
and the oracle's 64-spp feature buffers against the reference's pixel-centre rays.
"""
import numpy as np
import pytest

import _aov_ref as A
import _temporal_cases as K
import _temporal_closed as X
import _temporal_ref as T

f32 = np.float32


@pytest.fixture(scope="module")
def run(oracle_mod):
    def go(mode, W, H, cur_kw, prev_kw, bufs, **params):
        out, out_var, cls, (offered, used) = T.temporal(
            oracle_mod, T.camera(oracle_mod, W, H, mode, **cur_kw), T.camera(oracle_mod, W, H, mode, **prev_kw),
            mode=mode, return_taps=True, **bufs, **params)
        return X.Result(out, out_var, cls, offered, used)
    return go


# ---- the reference itself ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", X.MODES)
def test_project_inverts_pixel_ray(mode):
    rng = np.random.default_rng(3)
    for W, H in X.SIZES:
        for cam_kw in X.pairs(mode)["all"] + X.pairs(mode)["long"]:
            cam = X.camera(mode, W, H, **cam_kw)
            x, y, t = rng.random(200) * (W + 1) - 1, rng.random(200) * (H + 1) - 1, rng.random(200) * 30 + 0.5
            o, d = X.pixel_ray(cam, x, y)
            assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-14
            bx, by, depth, front = X.project(cam, o + d * t[:, None])
            assert front.all()
            assert max(np.abs(bx - x).max(), np.abs(by - y).max(), np.abs(depth - t).max()) < 1e-12


def test_the_basis_is_orthonormal_and_right_handed_and_the_near_plane_is_at_1():
    for mode in X.MODES:
        for cam_kw in X.pairs(mode)["long"]:
            cam = X.camera(mode, 37, 23, **cam_kw)
            R = cam["view"][:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
            fwd = -R[2]
            assert np.abs(np.cross(fwd, np.asarray(cam_kw["direction"], f32).astype(float))).max() < 1e-6
            assert R[1] @ np.asarray(cam_kw["up"], f32) > 0               # the image's up is the world's
            o, d = X.pixel_ray(cam, np.array([0.0, 36.0, 11.3]), np.array([0.0, 22.0, 4.9]))
            want = 1.0 if mode == "qe" else 0.0
            assert np.abs((o - cam["eye"]) @ fwd - want).max() < 1e-14
    # the field of view: CV horizontal over the width, QuinEngine vertical over the height; pixel W (H)
    # is one pixel past the last centre, so the frame spans [0, W] x [0, H] in these coordinates
    cv, qe = X.camera("cv", 64, 48, fov=50.0), X.camera("qe", 64, 48, fov=40.0)
    _, d = X.pixel_ray(cv, np.array([0.0, 64.0]), np.array([24.0, 24.0]))
    assert abs(np.degrees(np.arccos(d[0] @ d[1])) - 50.0) < 1e-9
    _, d = X.pixel_ray(qe, np.array([32.0, 32.0]), np.array([0.0, 48.0]))
    assert abs(np.degrees(np.arccos(d[0] @ d[1])) - 40.0) < 1e-9
    for cam in (cv, qe):                                              # square pixels in both
        _, d = X.pixel_ray(cam, np.array([32.0, 33.0, 32.0]), np.array([24.0, 24.0, 25.0]))
        assert abs(d[0] @ d[1] - d[0] @ d[2]) < 1e-12


def test_the_worlds_return_points_on_their_surfaces():
    cam = X.camera("qe", 37, 23, **X.DISOCCLUSION[0])
    fr = X.frame(cam, X.WorldWallPlate())
    assert set(np.unique(fr["sid"])) == {0, 1}
    assert np.abs(fr["P"][..., 2][fr["sid"] == 0] - 1).max() < 1e-12 and np.abs(fr["P"][..., 2][fr["sid"] == 1] - 9).max() < 1e-12
    plate = fr["P"][fr["sid"] == 1]
    assert np.abs(plate[:, 0]).max() <= 1.5 and np.abs(plate[:, 1] - 5).max() <= 1.5
    hinge = X.WorldWallPlate(hinge=70.0)
    fr = X.frame(cam, hinge)
    on = fr["sid"] == 1
    assert on.sum() >= 8 and np.abs((fr["P"][on] - hinge.c) @ hinge.n).max() < 1e-12
    assert abs(hinge.n @ np.array([0.0, 0.0, 1.0]) - np.cos(np.radians(70.0))) < 1e-12
    assert np.abs(fr["n"][on] @ np.array([0.0, 0.0, 1.0]) - np.cos(np.radians(70.0))).max() < 1e-12
    along = (fr["P"][on] - np.array([-1.5, 5.0, 1.0])) @ hinge.a          # from the edge on the wall
    assert along.min() >= 0 and along.max() <= 3 and np.abs(fr["P"][on][:, 1] - 5).max() <= 1.5
    shell = X.frame(cam, X.WorldShell((0.0, 5.0, 17.0)))
    assert np.abs(np.linalg.norm(shell["P"] - np.array([0.0, 5.0, 17.0]), axis=-1) - 14).max() < 1e-12
    assert np.abs((shell["n"] * (shell["P"] - np.array([0.0, 5.0, 17.0]))).sum(-1) + 14).max() < 1e-12
    plane = X.WorldPlane()
    fr = X.frame(cam, plane)
    assert np.abs((fr["P"] - plane.p) @ plane.n).max() < 1e-12 and (fr["n"] @ plane.n == 1).all()


# ---- on the restatement -------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["all", "dolly", "long"])
@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", X.MODES)
def test_reprojection_lands_where_the_projection_says(run, mode, size, pair):
    X.check_reprojection(run, mode, *size, *X.pairs(mode)[pair])


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


# ---- the oracle's frames ---------------------------------------------------------------------

@pytest.mark.parametrize("cam", sorted(X.RENDER_CAMERAS))
@pytest.mark.parametrize("mode", X.MODES)
def test_the_oracles_mean_depth_is_the_centre_rays(mcpt, oracle_mod, mode, cam):
    W, H = K.W0, K.H0
    cam_kw = X.RENDER_CAMERAS[cam]
    scene = (oracle_mod.Scene(mcpt.scene_path("qe_scene01"), flavor="tinyobj") if mode == "qe"
             else oracle_mod.Scene(mcpt.scene_path("scene01")))
    kw = dict(seed=K.QE_SEED, fresnel_kd=False) if mode == "qe" else {}
    ac, nd = A.aov_reference(oracle_mod, scene, W, H, X.RENDER_SPP, mode=mode, **kw, **cam_kw)
    o, d = X.centre_rays(mode, W, H, cam_kw)
    hits = A.first_hits(oracle_mod, scene, o, d, mode)
    X.check_centre_fit(ac, nd, hits["t"], hits["hit"], f"{mode} {cam}")
