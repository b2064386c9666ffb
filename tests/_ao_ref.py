"""numpy float32 restatement of the ambient-occlusion queries (csrc/ao.hip), built from
tests/_aov_ref.py (primary rays, first hits, normalize_cu) and the oracle's building
blocks: its RNG (orc_rng_init, orc_rng_next, orc_seed_key), its hemisphere sampler
(orc_sample_hemi) and its ordered KD walk for the closest hits.  A sample is occluded iff
its ray's closest hit exists with t < float32(radius).  Every float operation is one numpy
float32 operation in the kernel's order, so the GPU results are compared bit for bit.
"""
import ctypes as C

import numpy as np

from _aov_ref import first_hits, normalize_cu, primary_rays

f32 = np.float32
FLT_MAX = f32(3.402823466e38)
SEED = 0x4D435054
RENDER_BIAS = f32(0.01)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def stream_draws(oracle, ids, spp, spp_offset=0, seed=SEED, ndraws=4):
    """the first ndraws uniforms of sample spp_offset + s of stream id: (spp, n, ndraws) float32"""
    L = oracle.lib()
    key = L.orc_seed_key(C.c_uint64(seed))
    ids = np.asarray(ids, np.uint32).ravel()
    out = np.zeros((spp, ids.shape[0], ndraws), f32)
    st = C.c_uint32()
    for s in range(spp):
        for i, pid in enumerate(ids.tolist()):
            st.value = L.orc_rng_init(pid, key, (spp_offset + s) & 0xFFFFFFFF)
            for k in range(ndraws):
                out[s, i, k] = L.orc_rng_next(C.byref(st))
    return out


def hemi(oracle, nrm, u):
    """orc_sample_hemi (the reference's sampleHemi) of uniforms u (..., 2) about normals nrm (..., 3)"""
    oracle.lib()
    L = C.CDLL(oracle.LIB_PATH)
    L.orc_sample_hemi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    nrm = np.ascontiguousarray(np.broadcast_to(nrm, u.shape[:-1] + (3,)), f32)
    u = np.ascontiguousarray(u, f32)
    out = np.zeros(nrm.shape, f32)
    an, au, ao = nrm.ctypes.data, u.ctypes.data, out.ctypes.data
    for i in range(nrm.size // 3):
        L.orc_sample_hemi(an + 12 * i, au + 8 * i, ao + 12 * i)
    return out


def point_rays(oracle, p, nrm, ids, spp, spp_offset=0, seed=SEED, bias=0.0):
    """the point form's occlusion rays: origins and directions (spp, n, 3) float32 -- two
    draws dropped, the next two into the hemisphere about n_i, origin p_i + bias * h"""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, f32).reshape(-1, 3)
    u = stream_draws(oracle, ids, spp, spp_offset, seed)
    h = hemi(oracle, nrm[None], u[..., 2:4])
    b = RENDER_BIAS if bias == 0 else f32(bias)
    return (p[None] + h * b).astype(f32), h


def occluded(oracle, o_scene, o, d, radius, node_boxes=0):
    """bool array over the rays: the closest hit exists with t < float32(radius) (0: FLT_MAX)"""
    shape = o.shape[:-1]
    tri, _, hit, _ = o_scene.intersect(o.reshape(-1, 3), d.reshape(-1, 3), oracle.KD_ORDERED,
                                       node_boxes=node_boxes, threads=8)
    r = FLT_MAX if radius == 0 else f32(radius)
    return ((tri >= 0) & (hit[:, 2] < r)).reshape(shape)


def value(unocc, spp, prev=None, prev_count=0):
    """(float)unoccluded / (float)spp, then the linear running mean"""
    v = unocc.astype(f32) / f32(spp)
    if prev_count > 0:
        v = (np.asarray(prev, f32) * f32(prev_count) + v) / f32(prev_count + 1)
    return v.astype(f32)


def point_reference(oracle, o_scene, p, nrm, ids, spp, spp_offset=0, radius=0.0, bias=0.0, seed=SEED,
                    node_boxes=0, prev=None, prev_count=0):
    """mcpt_ao_device's output (n,) float32 and the occluded flags (spp, n)"""
    o, d = point_rays(oracle, p, nrm, ids, spp, spp_offset, seed, bias)
    occ = occluded(oracle, o_scene, o, d, radius, node_boxes)
    return value((~occ).sum(axis=0), spp, prev, prev_count), occ


def shading_normals(o_scene, hits):
    """normalize_cu of the interpolated vertex normals at the hits (zeros at a miss)"""
    ok = hits["hit"]
    tris = o_scene.triangles()[o_scene.kd_tris()[np.where(ok, hits["tri"], 0)]]
    nv = o_scene.normals()
    n1, n2, n3 = nv[tris[..., 6]], nv[tris[..., 7]], nv[tris[..., 8]]
    b, c = hits["beta"][..., None], hits["gamma"][..., None]
    n = normalize_cu(((n1 * (f32(1) - b - c) + n2 * b) + n3 * c).astype(f32))
    return np.where(ok[..., None], n, f32(0)).astype(f32)


def frame(oracle, o_scene, W, H, spp, spp_offset=0, seed=SEED, node_boxes=0, **cam):
    """What the pixel form knows of every sample before its occlusion ray, (spp, H, W[, 3])
    arrays: hit, the primary ray d, the hit point hp = o + t * d, the unflipped shading
    normal nrm, flip = dot(d, nrm) > 0, and the occlusion ray (origin, direction)"""
    o, d = primary_rays(oracle, W, H, spp, spp_offset=spp_offset, seed=seed, **cam)
    hits = first_hits(oracle, o_scene, o, d, "cv", node_boxes)
    ok = hits["hit"]
    nrm = shading_normals(o_scene, hits)
    flip = _dot(d, nrm) > 0
    pix = np.arange(W * H, dtype=np.uint32)
    u = stream_draws(oracle, pix, spp, spp_offset, seed).reshape(spp, H, W, 4)
    n_safe = np.where(ok[..., None], nrm, np.asarray([0, 1, 0], f32)).astype(f32)
    h = hemi(oracle, n_safe, u[..., 2:4])
    direc = np.where(flip[..., None], -h, h).astype(f32)
    t = np.where(ok, hits["t"], f32(0)).astype(f32)
    hp = (o + t[..., None] * d).astype(f32)
    oo = (hp + direc * RENDER_BIAS).astype(f32)
    return {"hit": ok, "d": d, "hp": hp, "nrm": nrm, "flip": flip & ok, "oo": oo, "od": direc}


def pixel_reference(oracle, o_scene, fr, radius, node_boxes=0, prev=None, prev_count=0):
    """mcpt_render_ao_device's output (H, W) float32 from frame()'s record, and the
    occluded flags (spp, H, W): a miss is unoccluded"""
    occ = occluded(oracle, o_scene, fr["oo"], fr["od"], radius, node_boxes) & fr["hit"]
    spp = occ.shape[0]
    return value((~occ).sum(axis=0), spp, prev, prev_count), occ
