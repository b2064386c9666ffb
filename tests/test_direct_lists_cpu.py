"""The wavefront's direct lists without a GPU (render_launch.hpp
"Direct lists"): the host's assignment of triangles to occluder boxes and the
small boxes' lists (capi.cpp build_image), and the decision -- the shade's
selector (trace_device.hpp scene_box_hits: exactly one box hit, and a small one)
followed by the extend's test of that box's triangles alone -- restated in
numpy float32 against the oracle's ordered walk.

For every ray the selector calls direct, the list's closest hit must be the
walk's hit id, misses included.  The triangle test is the oracle's (Math.hpp's
determinant, CUTracer.cu's Cramer quotients and acceptance, ties by rank),
operation for operation in float32, and the closest hit is the minimum of
(t, rank) over the triangles tested.  At least half of scene01's path-like
secondary rays that hit a box must be direct (priced 66%,
scripts/price_direct_lists.py).
"""
import os

import numpy as np
import pytest

from _raysets import ray_sets
from test_miss_cull_cpu import EPS_HI, EPS_LO, FLT_MAX, _adversarial_rays, _kd_verts, _path_like_rays

SCENES = ["scene01", "scene02", "scene03", "cornell_bunny70k"]


def box_hits(o, d, boxes, best=FLT_MAX):
    """trace_device.hpp scene_box_hits: may_hit_scene's slab test per box (float32,
    NaN-passing max / min, the 2^-12 margins) -> (boxes hit, index of the last one hit)"""
    o = np.asarray(o, np.float32)
    d = np.asarray(d, np.float32)
    count = np.zeros(len(o), np.int32)
    which = np.zeros(len(o), np.int32)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / d
        neg = np.signbit(d)
        for i, b in enumerate(np.asarray(boxes, np.float32)):
            lo = np.zeros(len(o), np.float32)
            hi = np.full(len(o), best, np.float32)
            for a in range(3):
                t0 = (np.where(neg[:, a], b[3 + a], b[a]) - o[:, a]) * inv[:, a]
                t1 = (np.where(neg[:, a], b[a], b[3 + a]) - o[:, a]) * inv[:, a]
                lo = np.fmax(lo, t0)
                hi = np.fmin(hi, t1)
            hit = ~(lo * EPS_LO > hi * EPS_HI)
            count += hit
            which = np.where(hit, i, which)
    return count, which


def _det3(m):
    """Math.hpp:169-175 (oracle orc_det3), float32, the same operand order; m[r][c] arrays"""
    r1 = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1])
    r2 = -m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
    r3 = m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0])
    return r1 + r2 + r3


def list_hit(o, d, tris, verts, prio):
    """closest hit of rays (o, d) over their candidate triangles tris (n, K) kd ids, -1 = none:
    CUTracer.cu:54-92 per triangle in float32, the minimum of (t, rank); -> kd id or -1"""
    n = len(o)
    best_t = np.full(n, FLT_MAX, np.float32)
    best_p = np.full(n, 0xFFFFFFFF, np.uint64)
    best = np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        for j in range(tris.shape[1]):
            k = tris[:, j]
            have = k >= 0
            v = verts[np.where(have, k, 0)]                     # (n, 3, 3)
            a, b, c = v[:, 0], v[:, 1], v[:, 2]
            ab, ac, ao = a - b, a - c, a - o
            rows = lambda x, y, z: [[x[:, r], y[:, r], z[:, r]] for r in range(3)]   # noqa: E731
            detA = _det3(rows(ab, ac, d))
            beta = _det3(rows(ao, ac, d)) / detA
            gamma = _det3(rows(ab, ao, d)) / detA
            t = _det3(rows(ab, ac, ao)) / detA
            p = prio[np.where(have, k, 0)].astype(np.uint64)
            ok = have & (beta + gamma < 1) & (beta > 0) & (gamma > 0) & (t > 0) & \
                ((t < best_t) | ((t == best_t) & (p < best_p)))
            best_t = np.where(ok, t, best_t)
            best_p = np.where(ok, p, best_p)
            best = np.where(ok, k, best)
    return best


def _kd_rank(osc):
    """kd id -> brute-force iteration rank (CUTracer.cu:49-54: geometries in order, each one's
    triangles in order), the tie-break of equal t"""
    rank_of = {}
    r = 0
    for g in osc.geoms():
        for cv in range(int(g[12]), int(g[12]) + int(g[13])):
            rank_of[cv] = r
            r += 1
    return np.array([rank_of[int(cv)] for cv in osc.kd_tris()], np.uint32)


# ---- the builder --------------------------------------------------------------------------

def check_builder_invariants(mcpt, name, path):
    """the assignment and the lists of one scene (shared with the scene zoo, tests/test_zoo_cpu.py)"""
    s, v = _kd_verts(mcpt, path)
    boxes = s.miss_cull_boxes()
    dl = s.direct_lists()
    k = dl["k"]
    assert k >= 1 and s.info()["direct_list_k"] == k
    assert len(dl["box_tris"]) == len(boxes) == s.info()["miss_cull_boxes"]
    if not len(boxes):                                     # (scene03: a closed room)
        assert s.info()["direct_list_boxes"] == 0 and not dl["counts"].any()
        return
    tb = dl["tri_box"]
    assert tb.shape == (len(v),) and tb.min() >= 0 and tb.max() < len(boxes)
    # every triangle is assigned to a box that holds its AABB
    b = boxes[tb]
    assert ((v >= b[:, None, :3]) & (v <= b[:, None, 3:])).all()
    assert np.array_equal(np.bincount(tb, minlength=len(boxes)), dl["box_tris"])
    # small boxes hold 1..k triangles and list exactly their own, in image (record) order
    small = np.flatnonzero(dl["counts"])
    assert s.info()["direct_list_boxes"] == len(small)
    for i in range(len(boxes)):
        n = int(dl["counts"][i])
        assert n == (dl["box_tris"][i] if 1 <= dl["box_tris"][i] <= k else 0)
        rec, kd = dl["lists"][i], dl["list_kd"][i]
        assert sorted(kd[:n]) == sorted(np.flatnonzero(tb == i)) if n else not rec.any()
        assert (kd[n:] == -1).all() and (rec[n:] == 0).all()
        assert (rec[:n] % 3 == 0).all() and (np.diff(rec[:n].astype(np.int64)) > 0).all()
        assert (rec[:n] < 3 * len(v)).all()
    if name == "scene01":                                  # the five walls, two triangles each
        assert len(small) == 5 and (dl["counts"][small] == 2).all()
    # the miss cull's report is what it was: the boxes do not depend on the lists
    again = mcpt.Scene(mcpt.ObjModel(path), host_only=True)
    assert again.miss_cull_boxes().tobytes() == boxes.tobytes()
    assert again.direct_lists()["lists"].tobytes() == dl["lists"].tobytes()


@pytest.mark.parametrize("name", SCENES)
def test_builder_invariants(mcpt, name):
    check_builder_invariants(mcpt, name, mcpt.scene_path(name))


@pytest.mark.parametrize("name", SCENES)
def test_miss_cull_boxes_are_what_they_were(mcpt, name):
    """mcpt_scene_miss_cull_boxes reports, bit for bit, the boxes recorded from the
    library before the lists existed (tests/golden/miss_cull_boxes.npz)"""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "miss_cull_boxes.npz"))
    for layout in ("auto", "global"):
        boxes = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name)), host_only=True, layout=layout).miss_cull_boxes()
        assert boxes.shape == gold[name].shape and boxes.tobytes() == gold[name].tobytes()


# ---- the decision -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene01_case(mcpt, oracle_mod):
    rng = np.random.default_rng(0x444C5354)
    path = mcpt.scene_path("scene01")
    osc = oracle_mod.Scene(path)
    s, verts = _kd_verts(mcpt, path)
    boxes = s.miss_cull_boxes()
    po, pd = _path_like_rays(oracle_mod, osc, rng, side=344)
    ao, ad = _adversarial_rays(boxes, rng)
    ro, rd = ray_sets(osc, 40000, 0x5EED)
    o, d = np.concatenate([po, ao, ro]), np.concatenate([pd, ad, rd])
    tri = osc.intersect(o, d, traversal=oracle_mod.KD_ORDERED, threads=8)[0]
    assert np.array_equal(verts, osc.kd_verts())               # the product's kd ids are the oracle's
    return s, osc, verts, boxes, o, d, tri, len(po)


def _selector(s, boxes, o, d):
    dl = s.direct_lists()
    count, which = box_hits(o, d, boxes)
    direct = (count == 1) & (dl["counts"][which] > 0)
    return direct, count, dl["list_kd"][which]


def test_direct_rays_get_the_walks_hit(scene01_case, oracle_mod):
    s, osc, verts, boxes, o, d, tri, n_path = scene01_case
    assert n_path >= 250000 and len(o) - n_path >= 60000
    direct, count, cand = _selector(s, boxes, o, d)
    assert direct[n_path:].sum() >= 5000 and (~direct[n_path:]).sum() >= 5000   # the adversarial rays fall on both sides
    prio = _kd_rank(osc)
    got = list_hit(o[direct], d[direct], cand[direct], verts, prio)
    bad = got != tri[direct]
    assert not bad.any(), (int(bad.sum()), o[direct][bad][:4], d[direct][bad][:4], got[bad][:4], tri[direct][bad][:4])
    assert (got >= 0).any() and (got < 0).any()                # hits and misses both


def test_at_least_half_of_the_walked_rays_are_direct(scene01_case):
    s, osc, verts, boxes, o, d, tri, n_path = scene01_case
    direct, count, _ = _selector(s, boxes, o[:n_path], d[:n_path])
    walked = count >= 1                                        # (the others: the miss cull takes them)
    share = direct.sum() / walked.sum()
    print("path-like rays %d: hit a box %d, direct %d (%.1f%% of those)" % (n_path, walked.sum(), direct.sum(), 100 * share))
    assert share >= 0.5


def test_one_box_rays_hit_only_that_boxes_triangles(scene01_case):
    """the argument itself, on every ray that hits exactly one box, small or not:
    the walk's hit triangle is assigned to that box"""
    s, osc, verts, boxes, o, d, tri, n_path = scene01_case
    count, which = box_hits(o, d, boxes)
    one = (count == 1) & (tri >= 0)
    assert one.sum() >= 100000
    assert np.array_equal(s.direct_lists()["tri_box"][tri[one]], which[one])
    assert not ((count == 0) & (tri >= 0)).any()
