"""numpy float32 restatement of the temporal accumulation (csrc/temporal.hip,
DESIGN.md section 17): every float operation is one numpy float32 operation in
the kernel's order and association, so the GPU results are compared bit for
bit.  The camera constants come from the oracle's host functions (its basis,
tan(fov / 2) and QuinEngine projection), which the feature-buffer suites
already pin against the library's.

Besides the outputs it returns a class per pixel: why it was reset, or which
of the two gathers gave it its history.
"""
import ctypes as C

import numpy as np

import _aov_ref as A

f32 = np.float32
MISS, BEHIND, REJECTED, BILINEAR, FALLBACK = 0, 1, 2, 3, 4
CLASS_NAMES = {MISS: "reset-miss", BEHIND: "reset-behind/off-screen", REJECTED: "reset-rejected",
               BILINEAR: "bilinear", FALLBACK: "fallback"}


def camera(oracle, W, H, mode="cv", fov=None, eye=(0.0, 5.0, 17.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
    """the constants the kernel takes for one frame: eye, fwd, up, right (float32 triples), th,
    proj11, proj22 (the projection: QuinEngine mode only)"""
    L = oracle.lib()
    fwd, upv, right = oracle.camera_basis(eye, direction, up)
    cam = {"eye": np.asarray(eye, f32), "fwd": fwd.astype(f32), "up": upv.astype(f32), "right": right.astype(f32),
           "th": f32(L.orc_tan_half_fov(C.c_float(60.0 if fov is None else fov))), "p11": f32(0), "p22": f32(0)}
    if mode == "qe":
        p11, p22 = C.c_float(), C.c_float()
        L.orc_qe_proj(C.c_float(45.0 if fov is None else fov), W, H, C.byref(p11), C.byref(p22))
        cam["p11"], cam["p22"] = f32(p11.value), f32(p22.value)
    return cam


def _dot(vx, vy, vz, b):
    return (vx * b[0] + vy * b[1]) + vz * b[2]


def reproject(cur, prev, albedo_cov, normal_depth, mode="cv"):
    """per pixel: hit (cov > 0), front (zc > 0), bx, by, the expected depth e -- garbage where
    the flags before them are false"""
    ac, nd = np.asarray(albedo_cov, f32), np.asarray(normal_depth, f32)
    H, W = ac.shape[:2]
    Wf, Hf = f32(W), f32(H)
    hw = Hf / Wf
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(f32), ys.astype(f32)
    cov = ac[..., 3]
    with np.errstate(all="ignore"):
        z = nd[..., 3] / cov
        if mode == "qe":
            idx = (f32(2) * xf / Wf - f32(1)) / cur["p11"]
            idy = (f32(1) - f32(2) * yf / Hf) / cur["p22"]
        else:
            idx = (f32(2) * xf / Wf - f32(1)) * cur["th"]
            idy = (hw - f32(2) * yf / Wf) * cur["th"]
        w = [(cur["right"][a] * idx + cur["up"][a] * idy) + cur["fwd"][a] for a in range(3)]
        ln = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        d = [w[a] / ln for a in range(3)]
        o = [(cur["eye"][a] + w[a]) if mode == "qe" else np.full((H, W), cur["eye"][a], f32) for a in range(3)]
        P = [o[a] + d[a] * z for a in range(3)]
        v = [P[a] - prev["eye"][a] for a in range(3)]
        zc = _dot(v[0], v[1], v[2], prev["fwd"])
        xv = _dot(v[0], v[1], v[2], prev["right"]) / zc
        yv = _dot(v[0], v[1], v[2], prev["up"]) / zc
        if mode == "qe":
            bx = ((xv * prev["p11"] + f32(1)) * f32(0.5)) * Wf
            by = ((f32(1) - yv * prev["p22"]) * f32(0.5)) * Hf
        else:
            bx = ((xv / prev["th"] + f32(1)) * f32(0.5)) * Wf
            by = ((hw - yv / prev["th"]) * f32(0.5)) * Wf
        l = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        e = (l - l / zc) if mode == "qe" else l
        hit = ~(cov <= f32(0))
        front = ~(zc <= f32(0))
    for a in (bx, by, e):
        assert a.dtype == f32
    return hit, front, bx.astype(f32), by.astype(f32), e.astype(f32)


def temporal(oracle, cur, prev, color, var, albedo_cov, normal_depth, hist_color_n, hist_var, hist_albedo_cov,
             hist_normal_depth, mode="cv", max_history=32, normal_threshold=0.9, sigma_z=0.1, gamma_space=False,
             return_taps=False):
    """csrc/temporal.hip in numpy float32.  cur / prev: camera(...) of the two frames; color
    (H, W, 3) or (H, W, 4); every other buffer (H, W, 4); var and hist_var both None: no
    variance.  Returns (out_color_n (H, W, 4), out_var (H, W, 4) or None, class (H, W) int);
    return_taps: also (the bilinear taps in the image with a weight > 0, those of them that
    contributed), each (H, W) int."""
    col = np.asarray(color, f32)[..., :3]
    H, W = col.shape[:2]
    if gamma_space:
        col = A._powf(oracle, col, A.QE_GAMMA)
    ac, nd = np.asarray(albedo_cov, f32), np.asarray(normal_depth, f32)
    hc, hac, hnd = np.asarray(hist_color_n, f32), np.asarray(hist_albedo_cov, f32), np.asarray(hist_normal_depth, f32)
    with_var = var is not None
    vv = np.asarray(var, f32)[..., :3] if with_var else None
    hv = np.asarray(hist_var, f32)[..., :3] if with_var else None
    thr, sz, Wf, Hf = f32(normal_threshold), f32(sigma_z), f32(W), f32(H)
    cov = ac[..., 3]

    hit, front, bx, by, e = reproject(cur, prev, ac, nd, mode)
    with np.errstate(all="ignore"):
        inside = (bx >= f32(-1)) & (bx <= Wf) & (by >= f32(-1)) & (by <= Hf)
    live = hit & front & inside                      # the pixels that gather

    sc = np.zeros((H, W, 4), f32)
    sw = np.zeros((H, W), f32)
    sv = np.zeros((H, W, 3), f32)
    offered = np.zeros((H, W), np.int32)
    used = np.zeros((H, W), np.int32)

    def tap(qx, qy, wk, active):
        nonlocal sc, sw, sv, offered, used
        with np.errstate(all="ignore"):
            ok = active & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H) & (wk > f32(0))
            offered = offered + ok
            jx, jy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            cq = hac[jy, jx, 3]
            nq = hnd[jy, jx]
            ok = ok & (cq > f32(0))
            dt = (nd[..., 0] * nq[..., 0] + nd[..., 1] * nq[..., 1]) + nd[..., 2] * nq[..., 2]
            ok = ok & (dt >= thr * (cov * cq))
            zq = nq[..., 3] / cq
            ok = ok & (np.abs(e - zq) <= sz * np.fmax(e, zq))
            used = used + ok
            sw = np.where(ok, sw + wk, sw).astype(f32)
            sc = np.where(ok[..., None], sc + wk[..., None] * hc[jy, jx], sc).astype(f32)
            if with_var:
                sv = np.where(ok[..., None], sv + (wk * wk)[..., None] * hv[jy, jx], sv).astype(f32)

    with np.errstate(all="ignore"):
        x0, y0 = np.floor(bx), np.floor(by)
        fx, fy = (bx - x0).astype(f32), (by - y0).astype(f32)
        gx, gy = f32(1) - fx, f32(1) - fy
        ix = np.where(live, x0, 0).astype(np.int64)
        iy = np.where(live, y0, 0).astype(np.int64)
        cx = np.where(live, np.floor(bx + f32(0.5)), 0).astype(np.int64)
        cy = np.where(live, np.floor(by + f32(0.5)), 0).astype(np.int64)
    tap(ix, iy, gx * gy, live)
    tap(ix + 1, iy, fx * gy, live)
    tap(ix, iy + 1, gx * fy, live)
    tap(ix + 1, iy + 1, fx * fy, live)
    bilinear = live & (sw > f32(0))
    taps = (offered.copy(), used.copy())
    fall = live & ~bilinear
    one = np.ones((H, W), f32)
    for ty in (-1, 0, 1):
        for tx in (-1, 0, 1):
            tap(cx + tx, cy + ty, one, fall)
    have = live & (sw > f32(0))

    cls = np.full((H, W), REJECTED, np.int32)
    cls[~hit] = MISS
    cls[hit & ~(front & inside)] = BEHIND
    cls[bilinear] = BILINEAR
    cls[fall & have] = FALLBACK

    with np.errstate(all="ignore"):
        h = (sc / sw[..., None]).astype(f32)
        ne = np.fmin(h[..., 3], f32(max_history - 1)).astype(f32)
        n1 = (ne + f32(1)).astype(f32)
        blend = ((h[..., :3] * ne[..., None] + col) / n1[..., None]).astype(f32)
        out = np.concatenate([col, np.ones((H, W, 1), f32)], axis=-1).astype(f32)
        out[have] = np.concatenate([blend, n1[..., None]], axis=-1)[have]
        out_var = None
        if with_var:
            hvar = (sv / (sw * sw)[..., None]).astype(f32)
            bv = (((hvar * ne[..., None]) * ne[..., None] + vv) / (n1 * n1)[..., None]).astype(f32)
            out_var = np.zeros((H, W, 4), f32)
            out_var[..., :3] = np.where(have[..., None], bv, vv)
    return (out, out_var, cls, taps) if return_taps else (out, out_var, cls)
