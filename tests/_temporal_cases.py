"""The frames the temporal-accumulation suites share: the camera pairs of the scene01 cases with
the classes (tests/_temporal_ref.py) each must populate -- tests/test_temporal_cpu.py asserts
that on the oracle's feature buffers, tests/test_gpu_temporal.py on the GPU's -- and the
synthetic frames of a wall seen from two cameras half a pixel apart.
"""
import math

import numpy as np

import _temporal_ref as T

f32 = np.float32
FEATURE_SPP = 4
QE_SEED = 822569775                  # the QuinEngine-mode frames' 32-bit frame seed
W0, H0 = 37, 23                      # neither a multiple of 16 or 8


def yaw(deg):
    """the default view direction turned by deg about the up axis"""
    a = math.radians(deg)
    return (math.sin(a), 0.0, -math.cos(a))


DEFAULT = dict(eye=(0.0, 5.0, 17.0), direction=(0.0, 0.0, -1.0))
ORBIT = dict(eye=(2.0, 6.5, 15.0), direction=(-0.1, -0.15, -1.0), up=(0.1, 1.0, 0.0))
# name: (mode, W, H, cur camera, prev camera, the classes the reference must populate)
SCENE_CASES = {
    "equal": ("cv", W0, H0, DEFAULT, DEFAULT, (T.MISS, T.REJECTED, T.BILINEAR)),
    "yaw2": ("cv", W0, H0, dict(eye=(0.0, 5.0, 17.0), direction=yaw(2.0)), DEFAULT,
             (T.MISS, T.REJECTED, T.BILINEAR, T.FALLBACK)),
    # one unit to the right: the wall behind the boxes' left edges comes into view
    "shift": ("cv", W0, H0, dict(eye=(1.0, 5.0, 17.0), direction=(0.0, 0.0, -1.0)), DEFAULT,
              (T.MISS, T.REJECTED, T.BILINEAR, T.FALLBACK)),
    "turn120": ("cv", W0, H0, DEFAULT, dict(eye=(0.0, 5.0, 17.0), direction=yaw(120.0)), (T.MISS, T.BEHIND)),
    "qe-yaw2": ("qe", W0, H0, dict(eye=(0.0, 5.0, 17.0), direction=yaw(2.0)), DEFAULT,
                (T.MISS, T.REJECTED, T.BILINEAR, T.FALLBACK)),
    # 4:3, and a zoom between the frames: the new frame's rim was outside the previous one
    "aspect-fov": ("cv", 64, 48, dict(eye=(0.0, 5.0, 17.0), direction=yaw(2.0), fov=50.0),
                   dict(eye=(0.0, 5.0, 17.0), direction=(0.0, 0.0, -1.0), fov=45.0),
                   (T.MISS, T.BEHIND, T.REJECTED, T.BILINEAR, T.FALLBACK)),
    # pitch, roll and an up that is not (0, 1, 0): camera_consts' basis with every input in play
    "orbit": ("cv", W0, H0, ORBIT, DEFAULT, (T.MISS, T.REJECTED, T.BILINEAR, T.FALLBACK)),
    "qe-orbit": ("qe", W0, H0, ORBIT, DEFAULT, (T.MISS, T.REJECTED, T.BILINEAR, T.FALLBACK)),
}


def history_lengths(H, W):
    """history lengths 1 .. 40 in a fixed pattern: some beyond the default cap of 32"""
    ys, xs = np.mgrid[0:H, 0:W]
    return (1 + (7 * xs + 3 * ys) % 40).astype(f32)


def populated(cls):
    return {k for k in range(5) if (cls == k).any()}


# ---- synthetic frames ----------------------------------------------------------------------
SYNTHETIC_SIZES = [(1, 1), (1, 17), (16, 16), (33, 65)]          # (W, H)
WALL_DISTANCE = 12.0
SYN_EYE = (0.0, 5.0, 17.0)


def synthetic_seed(W, H):
    return 100 * H + W


def _wall_depth(W, H, th):
    """hit distance of every pixel centre's CVMCTracer-mode ray on the wall z = eye.z - WALL_DISTANCE
    (the camera looks down -z, so fwd . d = 1 / |w|): plain data, float64 rounded once"""
    ys, xs = np.mgrid[0:H, 0:W]
    idx = (2.0 * xs / W - 1.0) * th
    idy = (H / W - 2.0 * ys / W) * th
    return (WALL_DISTANCE * np.sqrt(idx * idx + idy * idy + 1.0)).astype(f32)


def synthetic(oracle, W, H, seed):
    """A wall facing the camera, seen by two cameras half a pixel apart sideways, with seeded random
    colours, variances and history lengths.  The history's coverage is a checkerboard of 1 and 0
    (pixel (0, 0) covered) and half of its covered pixels show another surface (a normal at right
    angles): every bilinear footprint straddles a covered and an uncovered pixel, and where the
    covered one is the other surface the 3x3 fallback takes over.  Rejected history pixels hold
    NaN and infinities in every buffer the kernel may not read from them.
    Returns (cur, prev, buffers): the two reference cameras and the dict of the ten input arrays."""
    rng = np.random.default_rng(seed)
    cur_kw = dict(eye=SYN_EYE, direction=(0.0, 0.0, -1.0))
    cur = T.camera(oracle, W, H, "cv", **cur_kw)
    pixel = 2.0 * float(cur["th"]) * WALL_DISTANCE / W            # a pixel's width on the wall
    prev_kw = dict(eye=(SYN_EYE[0] + 0.5 * pixel, SYN_EYE[1], SYN_EYE[2]), direction=(0.0, 0.0, -1.0))
    prev = T.camera(oracle, W, H, "cv", **prev_kw)
    depth = _wall_depth(W, H, float(cur["th"]))              # the same for both: they only differ in eye.x
    ys, xs = np.mgrid[0:H, 0:W]
    one, zero = np.ones((H, W), f32), np.zeros((H, W), f32)

    ac = np.stack([rng.random((H, W)), rng.random((H, W)), rng.random((H, W)), one], -1).astype(f32)
    nd = np.stack([zero, zero, one, depth], -1).astype(f32)
    covered = ((xs + ys) % 2 == 0)
    other = covered & (rng.random((H, W)) < 0.5)                  # another surface: fails the normal test
    hac = np.stack([rng.random((H, W)), rng.random((H, W)), rng.random((H, W)), covered.astype(f32)], -1).astype(f32)
    hnd = np.stack([np.where(other, one, zero), zero, np.where(other, zero, one), depth], -1).astype(f32)
    color = rng.random((H, W, 4)).astype(f32)
    var = np.concatenate([rng.random((H, W, 3)) * 0.05, zero[..., None]], -1).astype(f32)
    hcol = np.concatenate([rng.random((H, W, 3)), rng.integers(1, 48, (H, W, 1))], -1).astype(f32)
    hvar = np.concatenate([rng.random((H, W, 3)) * 0.05, zero[..., None]], -1).astype(f32)
    rejected = ~covered | other
    poison = np.where(rng.random((H, W, 4)) < 0.5, np.nan, np.inf).astype(f32)
    poison[..., 0] = -np.inf
    hcol[rejected] = poison[rejected]
    hvar[rejected] = poison[rejected]
    hnd[~covered] = np.nan                                        # (never read: the coverage comes first)
    hac[~covered, :3] = np.nan
    bufs = dict(color=color, var=var, albedo_cov=ac, normal_depth=nd, hist_color_n=hcol, hist_var=hvar,
                hist_albedo_cov=hac, hist_normal_depth=hnd)
    return (cur, cur_kw), (prev, prev_kw), bufs
