"""numpy restatement of the direct-lighting queries (csrc/direct.hip), built from
tests/_ao_ref.py (the sample streams, the pixel form's first hits and shading normals),
tests/_aov_ref.py and the oracle's geoms(), kd_tris(), kd_verts() and ordered KD walk.
The light table is formed in numpy float64 as include/mcpt.h specifies it; everything
after it is one numpy float32 operation per device operation in the kernel's order, so
the GPU results are compared bit for bit.  A shadow ray is occluded iff its closest hit
exists with t < t_max.
"""
import numpy as np

from _ao_ref import RENDER_BIAS, SEED, frame, stream_draws
from _radiance_q import combine

f32 = np.float32
f64 = np.float64
PW_PI = f32(3.14159265359)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def light_table(o_scene):
    """the scene's light table: kd_ids (L,) int32 ascending, cdf (L,) float32, normals (L, 3)
    float32, area_total float32; and per light the vertices verts (L, 3, 3) and ka (L, 3)"""
    g = o_scene.geoms()
    verts = o_scene.kd_verts()
    # a geometry covers the OBJ triangles [start, start + count); a triangle is the first cover's
    of_obj = np.full(o_scene.triangles().shape[0], -1, np.int64)
    for i in range(g.shape[0] - 1, -1, -1):
        of_obj[int(g[i, 12]):int(g[i, 12]) + int(g[i, 13])] = i
    geom_of = of_obj[o_scene.kd_tris()]
    emit = (g[:, 0:3] > 0).any(axis=1)[geom_of]
    v = verts.astype(f64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=-1)
    ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    area = 0.5 * ln
    ids = np.nonzero(emit & (area > 0))[0].astype(np.int32)
    S, run = f64(0), []
    for k in ids:                      # the running sums, in table order
        S = S + area[k]
        run.append(S)
    run = np.asarray(run, f64)
    with np.errstate(all="ignore"):
        normals = (c[ids] / ln[ids][:, None]).astype(f32)
    return {"kd_ids": ids, "cdf": (run / S).astype(f32) if len(ids) else np.zeros(0, f32), "normals": normals,
            "area_total": f32(S), "verts": verts[ids], "ka": g[geom_of[ids], 0:3].astype(f32)}


def select(cdf, u):
    """j = min(#{k : cdf_k <= u}, L - 1)"""
    return np.minimum(np.searchsorted(cdf, u, side="right"), cdf.shape[0] - 1)


def samples(table, x, n, u, bias):
    """The per-sample record of points x (..., 3) with unit normals n (..., 3) and uniforms
    u (..., 3): the light j, the point y on it, valid, the shadow ray (o, d), t_max and g"""
    x = np.asarray(x, f32)
    n = np.asarray(n, f32)
    bias = f32(bias)
    j = select(table["cdf"], u[..., 0])
    su = np.sqrt(u[..., 1])
    beta = (su * (f32(1) - u[..., 2]))[..., None]
    gamma = (su * u[..., 2])[..., None]
    v = table["verts"][j]
    y = (v[..., 0, :] * (f32(1) - beta - gamma) + v[..., 1, :] * beta) + v[..., 2, :] * gamma
    w = y - x
    r2 = _dot(w, w)
    r = np.sqrt(r2)
    with np.errstate(all="ignore"):
        d = (w / r[..., None]).astype(f32)
        cx = _dot(n, d)
        cy = np.abs(_dot(table["normals"][j], d))
        valid = (cx > 0) & (cy > 0) & (r > f32(2) * bias)
        g = ((cx * cy) * table["area_total"]) / (PW_PI * r2)
    o = (x + d * bias).astype(f32)
    assert y.dtype == f32 and g.dtype == f32 and o.dtype == f32
    return {"j": j, "y": y, "valid": valid, "o": o, "d": d, "t_max": (r - f32(2) * bias).astype(f32),
            "g": np.where(valid, g, f32(0)).astype(f32)}


def closest_t(oracle, o_scene, rec, node_boxes=0):
    """(hit, t) of the closest hits of the valid shadow rays (the others: no hit)"""
    shape = rec["valid"].shape
    ok = rec["valid"].ravel()
    o = np.where(ok[:, None], rec["o"].reshape(-1, 3), f32(0)).astype(f32)
    d = np.where(ok[:, None], rec["d"].reshape(-1, 3), np.asarray([0, 1, 0], f32)).astype(f32)
    tri, _, hit, _ = o_scene.intersect(o, d, oracle.KD_ORDERED, node_boxes=node_boxes, threads=8)
    return ((tri >= 0) & ok).reshape(shape), hit[:, 2].reshape(shape)


def visible(oracle, o_scene, rec, node_boxes=0):
    """valid and not occluded: no closest hit with t < t_max"""
    hit, t = closest_t(oracle, o_scene, rec, node_boxes)
    return rec["valid"] & ~(hit & (t < rec["t_max"]))


def contributions(table, rec, vis, illum=10.0):
    """(..., 3) float32: g * (Ka * illum) of the visible samples, zeros of the others"""
    e = rec["g"][..., None] * (table["ka"][rec["j"]] * f32(illum))
    return np.where(vis[..., None], e, f32(0)).astype(f32)


def value(contrib, spp_chunk=0, prev=None, prev_count=0):
    """per-sample contributions (spp, ..., 3) -> the queries' output: summed in sample order
    inside chunks, the chunk sums in chunk order, / (float)spp, then the linear running mean"""
    v = combine([contrib[s] for s in range(contrib.shape[0])], spp_chunk)
    if prev_count > 0:
        v = (np.asarray(prev, f32) * f32(prev_count) + v) / f32(prev_count + 1)
    return v.astype(f32)


def point_samples(oracle, table, p, nrm, ids, spp, spp_offset=0, seed=SEED, bias=0.0):
    """the point form's per-sample record (spp, n, ...): two draws dropped, the next three used"""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, f32).reshape(-1, 3)
    u = stream_draws(oracle, ids, spp, spp_offset, seed, ndraws=5)
    return samples(table, p[None], nrm[None], u[..., 2:5], RENDER_BIAS if bias == 0 else f32(bias))


def point_reference(oracle, o_scene, table, p, nrm, ids, spp, spp_offset=0, spp_chunk=0, illum=10.0, bias=0.0,
                    seed=SEED, node_boxes=0, prev=None, prev_count=0):
    """mcpt_direct_device's output (n, 3) float32, the record and the visible flags (spp, n)"""
    rec = point_samples(oracle, table, p, nrm, ids, spp, spp_offset, seed, bias)
    vis = visible(oracle, o_scene, rec, node_boxes)
    return value(contributions(table, rec, vis, illum), spp_chunk, prev, prev_count), rec, vis


def pixel_samples(oracle, o_scene, table, W, H, spp, spp_offset=0, seed=SEED, node_boxes=0, **cam):
    """the pixel form's per-sample record (spp, H, W, ...) at the frame's first hits (a miss:
    invalid), and _ao_ref.frame's record of the primary rays"""
    fr = frame(oracle, o_scene, W, H, spp, spp_offset, seed, node_boxes, **cam)
    n = np.where(fr["flip"][..., None], -fr["nrm"], fr["nrm"]).astype(f32)
    n = np.where(fr["hit"][..., None], n, np.asarray([0, 1, 0], f32)).astype(f32)
    u = stream_draws(oracle, np.arange(W * H, dtype=np.uint32), spp, spp_offset, seed, ndraws=5).reshape(spp, H, W, 5)
    rec = samples(table, fr["hp"], n, u[..., 2:5], RENDER_BIAS)
    rec["valid"] = rec["valid"] & fr["hit"]
    rec["g"] = np.where(rec["valid"], rec["g"], f32(0)).astype(f32)
    return rec, fr


def pixel_reference(oracle, o_scene, table, rec, spp_chunk=0, illum=10.0, node_boxes=0, prev=None, prev_count=0):
    """mcpt_render_direct_device's output (H, W, 3) float32 from pixel_samples' record, and the
    visible flags (spp, H, W)"""
    vis = visible(oracle, o_scene, rec, node_boxes)
    return value(contributions(table, rec, vis, illum), spp_chunk, prev, prev_count), vis
