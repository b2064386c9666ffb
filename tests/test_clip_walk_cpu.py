"""The wavefront's clip walk without a GPU (render_launch.hpp "Clip walk"): the
decision -- the shade's selector (trace_device.hpp scene_box_hits as a box mask:
at least one box without a list, at most one with a list, not a direct ray) and
the extend's clip interval (box_interval over the selector's unlisted boxes:
[min lo * kEpsLo, max hi * kEpsHi]) -- restated in numpy float32 against the
oracle's ordered walk, on path-like and adversarial rays of scene01, scene02 and
the 70k mesh (the decision is the ray's and the boxes' alone, whatever layout the
product gives the scene).

For every selected ray the walk's hit must be a triangle of the selector's listed
box, or a triangle of one of its unlisted boxes at a t inside the clip interval,
or a miss: then the listed box's list plus the leaves a walk reaches inside the
interval hold the closest hit, and the minimum of (t, rank) over a superset of
the triangles a ray can hit is the walk's hit.  No triangle outside the
selector's boxes may be the hit.  At least 20% of scene01's path-like rays that
hit a box must be selected (priced 33%, scripts/price_clip_walk.py).
"""
import numpy as np
import pytest

from test_miss_cull_cpu import EPS_HI, EPS_LO, FLT_MAX, _adversarial_rays, _kd_verts, _path_like_rays

SCENES = {"scene01": 344, "scene02": 200, "cornell_bunny70k": 160}     # the primary grid's side


def box_intervals(o, d, boxes, best=FLT_MAX):
    """trace_device.hpp scene_box_hits / box_interval per box (float32, NaN-passing max / min):
    -> (hit (n, B) bool by the 2^-12 margins, lo (n, B), hi (n, B))"""
    o = np.asarray(o, np.float32)
    d = np.asarray(d, np.float32)
    n, nb = len(o), len(boxes)
    hit = np.zeros((n, nb), bool)
    los = np.zeros((n, nb), np.float32)
    his = np.zeros((n, nb), np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / d
        neg = np.signbit(d)
        for i, b in enumerate(np.asarray(boxes, np.float32)):
            lo = np.zeros(n, np.float32)
            hi = np.full(n, best, np.float32)
            for a in range(3):
                t0 = (np.where(neg[:, a], b[3 + a], b[a]) - o[:, a]) * inv[:, a]
                t1 = (np.where(neg[:, a], b[a], b[3 + a]) - o[:, a]) * inv[:, a]
                lo = np.fmax(lo, t0)
                hi = np.fmin(hi, t1)
            hit[:, i] = ~(lo * EPS_LO > hi * EPS_HI)
            los[:, i], his[:, i] = lo, hi
    return hit, los, his


def selector(hit, listed):
    """the shade's decision from the box mask: (selected, the mask's unlisted part, its listed part)"""
    unl = hit & ~listed[None, :]
    lst = hit & listed[None, :]
    direct = (hit.sum(axis=1) == 1) & (lst.sum(axis=1) == 1)
    sel = unl.any(axis=1) & (lst.sum(axis=1) <= 1) & ~direct
    return sel, unl, lst


@pytest.fixture(scope="module", params=list(SCENES))
def case(request, mcpt, oracle_mod):
    name = request.param
    rng = np.random.default_rng(0x434C4950)
    path = mcpt.scene_path(name)
    osc = oracle_mod.Scene(path)
    s, verts = _kd_verts(mcpt, path)
    assert np.array_equal(verts, osc.kd_verts())               # the product's kd ids are the oracle's
    boxes = s.miss_cull_boxes()
    po, pd = _path_like_rays(oracle_mod, osc, rng, side=SCENES[name])
    ao, ad = _adversarial_rays(boxes, rng)
    o, d = np.concatenate([po, ao]), np.concatenate([pd, ad])
    tri, _, h, _ = osc.intersect(o, d, traversal=oracle_mod.KD_ORDERED, threads=8)
    return name, s, boxes, o, d, tri, h[:, 2].astype(np.float32), len(po)


def test_selected_rays_hit_inside_their_boxes_and_interval(case):
    name, s, boxes, o, d, tri, t, n_path = case
    dl = s.direct_lists()
    listed = dl["counts"] > 0
    assert listed.any() and (~listed).any()
    hit, lo, hi = box_intervals(o, d, boxes)
    sel, unl, lst = selector(hit, listed)
    assert sel[:n_path].sum() >= 1000 and sel[n_path:].sum() >= 1000 and (~sel[n_path:]).sum() >= 1000
    with np.errstate(all="ignore"):
        clo = np.where(unl, lo, np.float32(np.inf)).min(axis=1) * EPS_LO
        chi = np.where(unl, hi, np.float32(-np.inf)).max(axis=1) * EPS_HI
    k = np.flatnonzero(sel & (tri >= 0))
    tb = dl["tri_box"][tri[k]]
    in_listed = lst[k, tb]
    in_unlisted = unl[k, tb]
    bad_box = ~(in_listed | in_unlisted)
    assert not bad_box.any(), (name, int(bad_box.sum()), o[k][bad_box][:4], d[k][bad_box][:4], tri[k][bad_box][:4])
    inside = (clo[k] <= t[k]) & (t[k] <= chi[k])
    bad_t = in_unlisted & ~inside
    assert not bad_t.any(), (name, int(bad_t.sum()), o[k][bad_t][:4], d[k][bad_t][:4], t[k][bad_t][:4],
                             clo[k][bad_t][:4], chi[k][bad_t][:4])
    # all three outcomes occur: a hit in the listed box, one in an unlisted box, a miss
    print("%s: %d rays, %d selected: %d hit their listed box, %d an unlisted one, %d nothing" %
          (name, len(o), sel.sum(), in_listed.sum(), in_unlisted.sum(), (sel & (tri < 0)).sum()))
    assert in_listed.any() and in_unlisted.any() and (sel & (tri < 0)).any()


def test_a_fifth_of_scene01s_walked_rays_are_selected(case):
    name, s, boxes, o, d, tri, t, n_path = case
    if name != "scene01":
        return
    hit, _, _ = box_intervals(o[:n_path], d[:n_path], boxes)
    sel, _, _ = selector(hit, s.direct_lists()["counts"] > 0)
    share = sel.sum() / hit.any(axis=1).sum()
    print("path-like rays %d: hit a box %d, selected %d (%.1f%% of those)" % (n_path, hit.any(axis=1).sum(), sel.sum(),
                                                                                 100 * share))
    assert n_path >= 250000 and share >= 0.2
