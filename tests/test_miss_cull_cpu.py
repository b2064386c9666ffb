"""The miss cull without a GPU: the host's occluder boxes (host_model.cpp
miss_cull_boxes) and the decision (trace_device.hpp may_hit_scene, restated in
numpy float32) against the oracle's closest hits.

A ray that fails every box must have no hit; on scene01's path-like secondary
rays the cull must fire for at least 10% (priced 14-22%,
scripts/price_miss_cull.py).
"""
import os

import numpy as np
import pytest

EPS_LO, EPS_HI = np.float32(0.999755859375), np.float32(1.000244140625)
FLT_MAX = np.float32(3.402823466e38)


def may_hit_scene(o, d, boxes, best=FLT_MAX):
    """trace_device.hpp may_hit_scene / slab_hit, operation for operation in
    float32: slab ends by the direction's sign, NaN-passing max / min (fmax /
    fmin, as v_max_f32 / v_min_f32), the 2^-12 margins."""
    o = np.asarray(o, np.float32)
    d = np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / d
        neg = np.signbit(d)
        hit = np.zeros(len(o), bool)
        for b in np.asarray(boxes, np.float32):
            lo = np.zeros(len(o), np.float32)
            hi = np.full(len(o), best, np.float32)
            for a in range(3):
                t0 = (np.where(neg[:, a], b[3 + a], b[a]) - o[:, a]) * inv[:, a]
                t1 = (np.where(neg[:, a], b[a], b[3 + a]) - o[:, a]) * inv[:, a]
                lo = np.fmax(lo, t0)
                hi = np.fmin(hi, t1)
            hit |= ~(lo * EPS_LO > hi * EPS_HI)
    return hit


def _host_scene(mcpt, name, **kw):
    return mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name)), host_only=True, **kw)


def _kd_verts(mcpt, path):
    m = mcpt.ObjModel(path)
    s = mcpt.Scene(m, host_only=True)
    return s, m.vertices()[m.triangles()[s.kd()[2]][:, :3]]          # (n_kd, 3, 3)


# ---- the builder --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["scene01", "scene02", "scene03", "cornell_bunny70k"])
def test_every_triangle_lies_in_a_box(mcpt, name):
    s, v = _kd_verts(mcpt, mcpt.scene_path(name))
    boxes = s.miss_cull_boxes()
    assert len(boxes) == s.info()["miss_cull_boxes"] <= 16
    if name in ("scene01", "scene02"):                # open boxes: the cull is on
        assert len(boxes) >= 2
    if len(boxes):
        inside = ((v[:, None, :, :] >= boxes[None, :, None, :3]) & (v[:, None, :, :] <= boxes[None, :, None, 3:]))
        assert inside.all(axis=(2, 3)).any(axis=1).all()          # all three vertices in one and the same box
        # bounds are vertex coordinates, unrounded
        coords = np.unique(v)
        assert np.isin(boxes, coords).all()
    again = _host_scene(mcpt, name).miss_cull_boxes()
    assert boxes.tobytes() == again.tobytes()                     # deterministic, bit for bit


def test_scene01_walls_stay_flat(mcpt):
    boxes = _host_scene(mcpt, "scene01").miss_cull_boxes()
    flat = boxes[((boxes[:, 3:] - boxes[:, :3]) == 0).any(axis=1)]
    assert len(flat) == 5                                         # floor, ceiling, back, left, right
    lo, hi = boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)
    assert not (flat[:, 2] == hi[2]).any()                        # no box over the opening (z = 5)
    assert hi[2] == 5.0 and lo[2] == -5.0
    # the global layout has the same boxes
    assert _host_scene(mcpt, "scene01", layout="global").miss_cull_boxes().tobytes() == boxes.tobytes()


def test_closed_room_and_degenerate_sets_get_no_boxes(mcpt, tmp_path):
    src = mcpt.scene_path("scene01")
    (tmp_path / "scene01.mtl").write_text(open(os.path.splitext(src)[0] + ".mtl").read())
    # (vertices 1-4 of scene01 are the corners of its opening)
    (tmp_path / "closed.obj").write_text(open(src).read() +
                                         "g pFront\nusemtl initialShadingGroup\nf 1/1/1 2/2/1 4/4/1 3/3/1\n")
    s = mcpt.Scene(mcpt.ObjModel(str(tmp_path / "closed.obj")), host_only=True)
    assert s.info()["miss_cull_boxes"] == 0
    # one triangle: its box is the scene bounds
    (tmp_path / "lone.obj").write_text("v -3 1 -2\nv 4 2 -1\nv 0 8 -4\nvn 0 0 1\ng tri\nf 1//1 2//1 3//1\n")
    s = mcpt.Scene(mcpt.ObjModel(str(tmp_path / "lone.obj")), host_only=True)
    assert s.info()["miss_cull_boxes"] == 0 and s.miss_cull_boxes().shape == (0, 6)


# ---- the decision -------------------------------------------------------------------------

def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _path_like_rays(oracle_mod, osc, rng, side=320, bounces=6):
    """secondary rays as the path loop makes them: a grid of primary rays from
    the C2 camera, then diffuse bounces from origins hp + 0.01 * dir"""
    eye = np.array([0.0, 5.0, 17.0], np.float32)
    th = np.tan(np.radians(30.0))
    u = (np.arange(side) + 0.5) / side * 2 - 1
    dx, dy = np.meshgrid(u * th, -u * th)
    d = _unit(np.stack([dx.ravel(), dy.ravel(), -np.ones(side * side)], 1))
    o = np.repeat(eye[None], len(d), 0)
    kv = osc.kd_verts()
    n_geo = np.cross(kv[:, 1] - kv[:, 0], kv[:, 2] - kv[:, 0])
    out_o, out_d = [], []
    for _ in range(bounces):
        tri, _, hit, _ = osc.intersect(o, d, traversal=oracle_mod.KD_ORDERED, threads=8)
        ok = tri >= 0
        hp, n, din = hit[ok, 3:6], _unit(n_geo[tri[ok]]), d[ok]
        n = np.where((np.einsum("ij,ij->i", n, din) > 0)[:, None], -n, n)     # facing the incoming ray
        w = _unit(rng.normal(size=hp.shape))
        w = np.where((np.einsum("ij,ij->i", w, n) < 0)[:, None], -w, w).astype(np.float32)
        d = w
        o = (hp + np.float32(0.01) * d).astype(np.float32)
        out_o.append(o)
        out_d.append(d)
    return np.concatenate(out_o), np.concatenate(out_d)


def _adversarial_rays(boxes, rng, per_box=1500):
    """origins exactly on box planes (with and without a zero direction
    component along the plane's axis), rays along box edges, rays through box
    corners, origins outside the scene bounds"""
    lo, hi = boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)
    O, D = [], []
    for b in boxes:
        corners = np.array([[b[3 * ((c >> a) & 1) + a] for a in range(3)] for c in range(8)], np.float32)
        n = per_box
        # on a plane of the box, anywhere over it and a little beyond
        p = (b[:3] + (b[3:] - b[:3]) * rng.uniform(-0.1, 1.1, (n, 3))).astype(np.float32)
        a = rng.integers(0, 3, n)
        p[np.arange(n), a] = np.where(rng.integers(0, 2, n) == 1, b[3 + a], b[a])
        d = _unit(rng.normal(size=(n, 3)))
        d[: n // 2][np.arange(n // 2), a[: n // 2]] = 0.0                   # half of them run in the plane
        d[: n // 4] = np.where(np.abs(d[: n // 4]) == np.abs(d[: n // 4]).max(axis=1, keepdims=True),
                               np.sign(d[: n // 4]), 0.0)                   # a quarter: axis-parallel
        O.append(p)
        D.append(d.astype(np.float32))
        # along the edges: from a corner (or before it, or past the far end) along +-axis
        c = corners[rng.integers(0, 8, n)]
        a = rng.integers(0, 3, n)
        d = np.zeros((n, 3), np.float32)
        d[np.arange(n), a] = rng.choice([-1.0, 1.0], n)
        o = c.copy()
        o[np.arange(n), a] += (rng.choice([0.0, -1.0, 1.0, 0.5], n) * (b[3 + a] - b[a] + 1.0)).astype(np.float32)
        O.append(o)
        D.append(d)
        # through the corners, from inside and outside the scene bounds
        c = corners[rng.integers(0, 8, n)]
        o = (lo - 2.0 + (hi - lo + 4.0) * rng.uniform(0, 1, (n, 3))).astype(np.float32)
        dd = c - o
        dd[: n // 2] = _unit(dd[: n // 2] + 1e-30)                          # half normalised, half exact differences
        O.append(o)
        D.append(dd.astype(np.float32))
    # origins outside the bounds, aimed at the scene and away from it
    n = 20000
    o = (lo - 6.0 + (hi - lo + 12.0) * rng.uniform(0, 1, (n, 3))).astype(np.float32)
    o = o[((o < lo) | (o > hi)).any(axis=1)]
    t = (lo + (hi - lo) * rng.uniform(-0.2, 1.2, (len(o), 3))).astype(np.float32)
    O.append(o)
    D.append(_unit(t - o))
    O, D = np.concatenate(O), np.concatenate(D)
    keep = np.abs(D).max(axis=1) > 0
    return O[keep], D[keep]


@pytest.fixture(scope="module")
def scene01_rays(mcpt, oracle_mod):
    rng = np.random.default_rng(0x4D435054)
    path = mcpt.scene_path("scene01")
    osc = oracle_mod.Scene(path)
    boxes = mcpt.Scene(mcpt.ObjModel(path), host_only=True).miss_cull_boxes()
    po, pd = _path_like_rays(oracle_mod, osc, rng)
    ao, ad = _adversarial_rays(boxes, rng)
    o, d = np.concatenate([po, ao]), np.concatenate([pd, ad])
    tri = osc.intersect(o, d, traversal=oracle_mod.KD_ORDERED, threads=8)[0]
    return boxes, o, d, tri, len(po)


def test_no_culled_ray_has_a_hit(scene01_rays):
    boxes, o, d, tri, n_path = scene01_rays
    assert len(o) >= 200000 and n_path >= 150000
    culled = ~may_hit_scene(o, d, boxes)
    assert culled[n_path:].any() and (~culled[n_path:]).any()     # the adversarial rays fall on both sides
    bad = culled & (tri >= 0)
    assert not bad.any(), (int(bad.sum()), o[bad][:4], d[bad][:4])


def test_the_cull_is_not_vacuous(scene01_rays):
    boxes, o, d, tri, n_path = scene01_rays
    culled = ~may_hit_scene(o[:n_path], d[:n_path], boxes)
    miss = tri[:n_path] < 0
    print("path-like rays %d: miss %.1f%%, failing every box %.1f%%" % (n_path, 100 * miss.mean(), 100 * culled.mean()))
    assert culled.mean() >= 0.10


def test_ordered_walk_agrees_with_brute_force_on_culled_rays(scene01_rays, mcpt, oracle_mod):
    """the walk's miss is a true miss: brute force over every triangle finds nothing either"""
    boxes, o, d, tri, n_path = scene01_rays
    culled = np.flatnonzero(~may_hit_scene(o, d, boxes))[:20000]
    osc = oracle_mod.Scene(mcpt.scene_path("scene01"))
    assert (osc.intersect(o[culled], d[culled], traversal=oracle_mod.BRUTE, threads=8)[0] < 0).all()
