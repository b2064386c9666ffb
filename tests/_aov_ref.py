"""numpy float32 restatement of the first-hit feature buffers (csrc/aov.hip) and
of the a-trous denoiser (csrc/denoise.hip), built from the oracle's building
blocks: its RNG, camera and pow, and its ordered KD walk for the closest hits.
Every float operation is one numpy float32 (or, for the CVMCTracer
reprojection, float64) operation in the kernels' order, so the GPU results are
compared bit for bit.
"""
import ctypes as C

import numpy as np

f32 = np.float32
FLT_EPS = f32(1.192092896e-07)
QE_GAMMA = f32(2.2)
QE_INV_GAMMA = f32(0.454545454545)
QE_T_BEST = f32(10000.0)


def _draws(oracle, seeds, n):
    """n Park-Miller uniforms from each start state: (len(seeds), n) float32"""
    L = oracle.lib()
    out = np.zeros((len(seeds), n), f32)
    st = C.c_uint32()
    for i, sd in enumerate(seeds):
        st.value = int(sd)
        for k in range(n):
            out[i, k] = L.orc_rng_next(C.byref(st))
    return out


def _rot(right, up, fwd, vx, vy, vz):
    """right * vx + up * vy - fwd * vz per component, in the kernels' order"""
    return np.stack([(f32(right[a]) * vx + f32(up[a]) * vy) - f32(fwd[a]) * vz for a in range(3)], axis=-1)


def _len(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def normalize_cu(v):
    ln = _len(v)
    ok = np.abs(ln) > FLT_EPS
    with np.errstate(all="ignore"):
        return np.where(ok[..., None], v / np.where(ok, ln, f32(1))[..., None], v).astype(f32)


def normalize_hlsl(v):
    with np.errstate(all="ignore"):
        return (v / _len(v)[..., None]).astype(f32)


def primary_rays(oracle, W, H, spp, spp_offset=0, seed=0x4D435054, mode="cv", fov=None,
                 eye=(0.0, 5.0, 17.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
    """The renders' primary rays: origins and directions (spp, H, W, 3) float32.
    cv: rng_init(pixel, key, sample), +-1 px jitter, double reprojection 2 b / W
    (CUTracer.cu:186-211); qe: TEA-16(pixel, frame seed + sample), two warm-up
    draws, +-0.5 px jitter, near-plane origin (rtx.hlsl:380-397)."""
    L = oracle.lib()
    fwd, upv, right = oracle.camera_basis(eye, direction, up)
    ys, xs = np.mgrid[0:H, 0:W]
    pix = (ys * W + xs).astype(np.uint32).ravel()
    fx = np.broadcast_to(xs.astype(np.uint32).astype(f32), (spp, H, W))
    fy = np.broadcast_to(ys.astype(np.uint32).astype(f32), (spp, H, W))
    if mode == "cv":
        key = L.orc_seed_key(C.c_uint64(seed))
        seeds = [L.orc_rng_init(int(p), key, (spp_offset + s) & 0xFFFFFFFF) for s in range(spp) for p in pix]
        u = _draws(oracle, seeds, 2).reshape(spp, H, W, 2)
        bx = fx + (u[..., 0] * f32(2) - f32(1))
        by = fy + (u[..., 1] * f32(2) - f32(1))
        th = np.float64(L.orc_tan_half_fov(C.c_float(60.0 if fov is None else fov)))
        Wd, Hd = np.float64(W), np.float64(H)
        idx = ((2.0 * bx.astype(np.float64) / Wd - 1) * th).astype(f32)
        idy = ((1.0 * Hd / Wd - 2.0 * by.astype(np.float64) / Wd) * th).astype(f32)
        d = normalize_cu(_rot(right, upv, fwd, idx, idy, f32(-1)))
        o = np.broadcast_to(np.asarray(eye, f32), d.shape).copy()
        return o, d
    key = seed & 0xFFFFFFFF
    seeds = [L.orc_tea16(int(p), (key + spp_offset + s) & 0xFFFFFFFF) for s in range(spp) for p in pix]
    u = _draws(oracle, seeds, 4).reshape(spp, H, W, 4)
    p11, p22 = C.c_float(), C.c_float()
    L.orc_qe_proj(C.c_float(45.0 if fov is None else fov), W, H, C.byref(p11), C.byref(p22))
    bx = fx + (u[..., 2] - f32(0.5))
    by = fy + (u[..., 3] - f32(0.5))
    vx = (f32(2) * bx / f32(W) - f32(1)) / f32(p11.value)
    vy = (f32(1) - f32(2) * by / f32(H)) / f32(p22.value)
    w = _rot(right, upv, fwd, vx, vy, f32(-1))
    o = (w + np.asarray(eye, f32)).astype(f32)
    return o, normalize_hlsl(w)


def first_hits(oracle, o_scene, o, d, mode="cv", node_boxes=0):
    """Closest hits of the rays through the ordered KD walk: dict of (spp, H, W)
    arrays hit, geom, tri (kd id), beta, gamma, t"""
    shape = o.shape[:-1]
    tri, geom, hit, _ = o_scene.intersect(o.reshape(-1, 3), d.reshape(-1, 3), oracle.KD_ORDERED,
                                          node_boxes=node_boxes, threads=8)
    ok = tri >= 0
    if mode == "qe":
        ok &= hit[:, 2] < QE_T_BEST          # t_best starts at 10000 (rtx.hlsl:88)
    return {"hit": ok.reshape(shape), "geom": geom.reshape(shape), "tri": tri.reshape(shape),
            "beta": hit[:, 0].reshape(shape), "gamma": hit[:, 1].reshape(shape), "t": hit[:, 2].reshape(shape)}


def _mean_in_order(per_sample):
    """plain fp32 sum over axis 0 in order, from 0, divided by (float)spp"""
    acc = np.zeros(per_sample.shape[1:], f32)
    for s in range(per_sample.shape[0]):
        acc = acc + per_sample[s]
    return acc / f32(per_sample.shape[0])


def emission(o_scene, hits, illum=10.0):
    """mean of color * (Ka * illum) at the first hit, color = 1: a max_depth = 0 render"""
    g = o_scene.geoms()
    ka = g[np.where(hits["hit"], hits["geom"], 0)][..., 0:3].astype(f32)
    e = np.where(hits["hit"][..., None], f32(1) * (ka * f32(illum)), f32(0)).astype(f32)
    return _mean_in_order(e)


def aov(o_scene, hits, mode="cv", fresnel_kd=True, prev=None, prev_count=0):
    """(albedo_cov, normal_depth), each (H, W, 4) float32, as csrc/aov.hip forms them"""
    ok = hits["hit"]
    g = o_scene.geoms()[np.where(ok, hits["geom"], 0)].astype(f32)
    ka, kd, ks, ns, tr = g[..., 0:3], g[..., 3:6], g[..., 6:9], g[..., 9], g[..., 10]
    one = np.ones_like(kd)
    emit = (ka > 0).any(axis=-1)
    tint = kd if (fresnel_kd and mode == "cv") else one
    alb = np.where(emit[..., None], one,
                   np.where((tr > 0)[..., None], tint, np.where((ns > 1)[..., None], ks, kd)))
    tris = o_scene.triangles()[o_scene.kd_tris()[np.where(ok, hits["tri"], 0)]]
    nrm = o_scene.normals()
    n1, n2, n3 = nrm[tris[..., 6]], nrm[tris[..., 7]], nrm[tris[..., 8]]
    b, c = hits["beta"][..., None], hits["gamma"][..., None]
    n = (n1 * (f32(1) - b - c) + n2 * b) + n3 * c
    n = normalize_hlsl(n) if mode == "qe" else normalize_cu(n)
    z = np.zeros_like(n)
    ac = np.concatenate([np.where(ok[..., None], alb, z), ok[..., None].astype(f32)], axis=-1).astype(f32)
    nd = np.concatenate([np.where(ok[..., None], n, z), np.where(ok, hits["t"], f32(0))[..., None]],
                        axis=-1).astype(f32)
    ac, nd = _mean_in_order(ac), _mean_in_order(nd)
    if prev_count > 0:
        pc, pc1 = f32(prev_count), f32(prev_count + 1)
        ac = (prev[0] * pc + ac) / pc1
        nd = (prev[1] * pc + nd) / pc1
    return ac.astype(f32), nd.astype(f32)


def aov_reference(oracle, o_scene, W, H, spp, mode="cv", node_boxes=0, fresnel_kd=True, prev=None, prev_count=0,
                  **ray_kw):
    o, d = primary_rays(oracle, W, H, spp, mode=mode, **ray_kw)
    return aov(o_scene, first_hits(oracle, o_scene, o, d, mode, node_boxes), mode, fresnel_kd, prev, prev_count)


def _powf(oracle, a, y):
    L = oracle.lib()
    flat = a.astype(f32).ravel()
    out = np.array([L.orc_powf(C.c_float(float(v)), C.c_float(float(y))) for v in flat], f32)
    return out.reshape(a.shape)


H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)


def denoise(oracle, color, albedo_cov, normal_depth, iterations=5, normal_power_log2=7, sigma_z=0.1,
            albedo_floor=0.01, gamma_space=False):
    """csrc/denoise.hip in numpy float32, the same operations in the same order;
    color (H, W, 3), features (H, W, 4); returns (H, W, 3)"""
    col = np.asarray(color, f32)
    H, W = col.shape[:2]
    if gamma_space:
        col = _powf(oracle, col, QE_GAMMA)
    alb = np.maximum(np.asarray(albedo_cov, f32)[..., :3], f32(albedo_floor))
    c = (col / alb).astype(f32)
    n = np.asarray(normal_depth, f32)[..., :3]
    z = np.asarray(normal_depth, f32)[..., 3]
    for i in range(iterations):
        step = 1 << i
        sc = np.zeros_like(c)
        sw = np.zeros((H, W), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                h = H5[dy + 2] * H5[dx + 2]
                if dy == 0 and dx == 0:
                    w = np.full((y1 - y0, x1 - x0), h, f32)
                else:
                    np_, nq = n[P], n[Q]
                    dt = (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2]
                    wn = np.minimum(np.maximum(dt, f32(0)), f32(1))
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    r = np.abs(z[P] - z[Q]) / (f32(sigma_z) * np.maximum(z[P], z[Q]) + f32(1e-6))
                    m = np.maximum(f32(1) - r, f32(0))
                    w = (h * wn) * (m * m)
                sc[P] = sc[P] + w[..., None] * c[Q]
                sw[P] = sw[P] + w
        c = (sc / sw[..., None]).astype(f32)
    out = (c * alb).astype(f32)
    if gamma_space:
        out = _powf(oracle, out, QE_INV_GAMMA)
    return out
