"""The scene zoo (tests/_zoo.py) without a GPU: what each scene is for, as exact
facts about its occluder boxes and lists, and the secondary-ray decision -- the
shade's box mask, the direct rays' lists, the clip walk's interval -- restated in
numpy float32 (tests/test_direct_lists_cpu.py, tests/test_clip_walk_cpu.py) against
the oracle's ordered walk, on path-like rays (a 96 x 96 grid of primaries and six
diffuse bounces) and adversarial rays of every zoo scene.

The coverage tests count, on the oracle's own rays, the rays that take each branch
the zoo is for: tests/test_gpu_zoo.py renders the same scenes, and these floors are
why its image comparisons mean something.  Each floor is at most half of the count
measured when the scenes were made (in the tests' docstrings).
"""
import numpy as np
import pytest

from _zoo import ZOO, tri_groups, zoo_scenes  # noqa: F401  (zoo_scenes: a fixture)
from test_clip_walk_cpu import box_intervals, selector
from test_direct_lists_cpu import _kd_rank, box_hits, check_builder_invariants, list_hit
from test_miss_cull_cpu import EPS_HI, EPS_LO, _adversarial_rays, _kd_verts, _path_like_rays

SIDE = 96


def _host(mcpt, path):
    m = mcpt.ObjModel(path)
    return m, mcpt.Scene(m, host_only=True)


def _group_box(m, s, group):
    """the one occluder box that holds every triangle of an OBJ group"""
    names = sorted(m.groups())
    b = np.unique(s.direct_lists()["tri_box"][tri_groups(m, s) == names.index(group)])
    assert len(b) == 1, (group, b)
    return int(b[0])


# ---- what the scenes are ------------------------------------------------------------------

@pytest.mark.parametrize("name", ZOO)
def test_every_scene_is_in_lds_with_lists(mcpt, zoo_scenes, name):  # noqa: F811
    i = _host(mcpt, zoo_scenes[name])[1].info()
    assert i["node_boxes"] == 0 and i["direct_list_boxes"] > 0 and i["terminal_cull_boxes"] >= 1
    assert i["direct_list_k"] == 2


def test_single_has_only_lists_of_one(mcpt, zoo_scenes):  # noqa: F811
    m, s = _host(mcpt, zoo_scenes["single"])
    dl = s.direct_lists()
    assert sorted(dl["counts"]) == [0, 0, 1, 1] and sorted(dl["box_tris"]) == [1, 1, 3, 3]
    assert dl["counts"][_group_box(m, s, "tri")] == 1 and dl["counts"][_group_box(m, s, "lamp")] == 1


def test_tetras_has_one_list_and_overlapping_unlisted_boxes(mcpt, zoo_scenes):  # noqa: F811
    m, s = _host(mcpt, zoo_scenes["tetras"])
    dl, boxes = s.direct_lists(), s.miss_cull_boxes()
    listed = dl["counts"] > 0
    assert listed.sum() == 1 and listed[_group_box(m, s, "light")]
    assert (~listed).sum() >= 6 and s.info()["miss_cull_boxes"] <= 8
    pairs = 0
    unl = np.flatnonzero(~listed)
    for i in unl:
        for j in unl[unl > i]:
            a, b = boxes[i], boxes[j]
            overlap = (np.minimum(a[3:], b[3:]) > np.maximum(a[:3], b[:3])).all()     # a volume in common
            a_in_b = (a[:3] >= b[:3]).all() and (a[3:] <= b[3:]).all()
            b_in_a = (b[:3] >= a[:3]).all() and (b[3:] <= a[3:]).all()
            pairs += bool(overlap and not a_in_b and not b_in_a)
    assert pairs >= 1


def test_panes_lists_the_wall_both_panes_and_the_light(mcpt, zoo_scenes):  # noqa: F811
    m, s = _host(mcpt, zoo_scenes["panes"])
    assert s.direct_lists()["counts"].tolist() == [0, 2, 2, 2, 2]
    assert len({_group_box(m, s, g) for g in ("wall", "glass", "mirror", "light")}) == 4


def test_many_has_boxes_merged_at_a_cost(mcpt, zoo_scenes):  # noqa: F811
    m, s = _host(mcpt, zoo_scenes["many"])
    dl = s.direct_lists()
    assert s.info()["miss_cull_boxes"] == 8
    g = tri_groups(m, s)
    merged = [b for b in range(8) if dl["box_tris"][b] >= 4 and len(np.unique(g[dl["tri_box"] == b])) > 1]
    assert len(merged) >= 2
    assert (dl["counts"] > 0).sum() >= 2


@pytest.mark.parametrize("name", ZOO)
def test_builder_invariants(mcpt, zoo_scenes, name):  # noqa: F811
    check_builder_invariants(mcpt, name, zoo_scenes[name])


# ---- the decision -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def zoo_cases(mcpt, oracle_mod, zoo_scenes):  # noqa: F811
    """name -> the scene's rays, the walk's hits and the decision's parts, computed once and read-only"""
    have = {}

    def get(name):
        if name not in have:
            rng = np.random.default_rng(0x434C4950)                  # (test_clip_walk_cpu.py's seed)
            path = zoo_scenes[name]
            osc = oracle_mod.Scene(path)
            s, verts = _kd_verts(mcpt, path)
            assert np.array_equal(verts, osc.kd_verts())           # the product's kd ids are the oracle's
            boxes = s.miss_cull_boxes()
            po, pd = _path_like_rays(oracle_mod, osc, rng, side=SIDE)
            ao, ad = _adversarial_rays(boxes, rng)
            o, d = np.concatenate([po, ao]), np.concatenate([pd, ad])
            tri, _, h, _ = osc.intersect(o, d, traversal=oracle_mod.KD_ORDERED, threads=8)
            dl = s.direct_lists()
            listed = dl["counts"] > 0
            hit, lo, hi = box_intervals(o, d, boxes)
            sel, unl, lst = selector(hit, listed)
            count, which = box_hits(o, d, boxes)
            assert np.array_equal(count, hit.sum(axis=1))          # the two restatements of the box test agree
            direct = (count == 1) & listed[which]
            assert not (direct & sel).any()
            c = dict(name=name, s=s, m=mcpt.ObjModel(path), osc=osc, verts=verts, boxes=boxes, o=o, d=d, tri=tri,
                     t=h[:, 2].astype(np.float32), n_path=len(po), dl=dl, listed=listed, hit=hit, lo=lo, hi=hi,
                     sel=sel, unl=unl, lst=lst, count=count, which=which, direct=direct)
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            have[name] = c
        return have[name]

    return get


@pytest.mark.parametrize("name", ZOO)
def test_direct_rays_get_the_walks_hit(zoo_cases, name):
    """a direct ray's list (of one triangle in `single`) gives the walk's hit id, misses included,
    and no ray that fails every box has a hit"""
    c = zoo_cases(name)
    k = c["direct"]
    assert k[: c["n_path"]].any() and k[c["n_path"]:].sum() >= 500 and (~k[c["n_path"]:]).sum() >= 500
    got = list_hit(c["o"][k], c["d"][k], c["dl"]["list_kd"][c["which"][k]], c["verts"], _kd_rank(c["osc"]))
    bad = got != c["tri"][k]
    assert not bad.any(), (name, int(bad.sum()), c["o"][k][bad][:4], c["d"][k][bad][:4], got[bad][:4],
                           c["tri"][k][bad][:4])
    assert (got >= 0).any() and (got < 0).any()                    # hits and misses both
    culled = c["count"] == 0
    assert culled.any() and not (culled & (c["tri"] >= 0)).any()


@pytest.mark.parametrize("name", ZOO)
def test_selected_rays_hit_inside_their_boxes_and_interval(zoo_cases, name):
    """a selected ray's hit is a triangle of its listed box, or one of an unlisted box of its mask
    at a t inside the clip interval"""
    c = zoo_cases(name)
    sel, unl, lst, tri, t = c["sel"], c["unl"], c["lst"], c["tri"], c["t"]
    with np.errstate(all="ignore"):
        clo = np.where(unl, c["lo"], np.float32(np.inf)).min(axis=1) * EPS_LO
        chi = np.where(unl, c["hi"], np.float32(-np.inf)).max(axis=1) * EPS_HI
    k = np.flatnonzero(sel & (tri >= 0))
    assert len(k) >= 1000
    tb = c["dl"]["tri_box"][tri[k]]
    in_listed, in_unlisted = lst[k, tb], unl[k, tb]
    bad_box = ~(in_listed | in_unlisted)
    assert not bad_box.any(), (name, int(bad_box.sum()), c["o"][k][bad_box][:4], c["d"][k][bad_box][:4],
                               tri[k][bad_box][:4])
    bad_t = in_unlisted & ~((clo[k] <= t[k]) & (t[k] <= chi[k]))
    assert not bad_t.any(), (name, int(bad_t.sum()), c["o"][k][bad_t][:4], c["d"][k][bad_t][:4], t[k][bad_t][:4],
                             clo[k][bad_t][:4], chi[k][bad_t][:4])
    print("%s: %d rays, %d selected: %d hit their listed box, %d an unlisted one, %d nothing" %
          (name, len(tri), sel.sum(), in_listed.sum(), in_unlisted.sum(), (sel & (tri < 0)).sum()))
    assert in_unlisted.any() and (sel & (tri < 0)).any()


@pytest.mark.parametrize("name", ZOO)
def test_one_box_rays_hit_only_that_boxes_triangles(zoo_cases, name):
    c = zoo_cases(name)
    one = (c["count"] == 1) & (c["tri"] >= 0)
    assert one.sum() >= 1000
    assert np.array_equal(c["dl"]["tri_box"][c["tri"][one]], c["which"][one])


# ---- coverage: the rays the GPU tests are for exist -----------------------------------------

def _direct_on(c, group):
    """the path-like direct rays on a group's box: (rays, of them with a hit)"""
    n = c["n_path"]
    k = c["direct"][:n] & (c["which"][:n] == _group_box(c["m"], c["s"], group))
    return int(k.sum()), int((k & (c["tri"][:n] >= 0)).sum())


def _unlisted_in_mask(c):
    return c["unl"][c["sel"]].sum(axis=1)


def test_single_sends_rays_through_both_one_triangle_lists(zoo_cases):
    """measured: 451 path-like direct rays on the red triangle's box (76 hit it) and 63 on the emitting
    triangle's (30 hit it)"""
    c = zoo_cases("single")
    for group in ("tri", "lamp"):
        n, hits = _direct_on(c, group)
        print("single: %d path-like direct rays on %s, %d hit it" % (n, group, hits))
        assert n >= 30 and 0 < hits < n


def test_tetras_joins_intervals_over_many_unlisted_boxes(zoo_cases):
    """measured: of 30 957 selected rays, 10 204 / 3 540 / 730 / 32 have 2 / 3 / 4 / 5 unlisted boxes in their mask"""
    c = zoo_cases("tetras")
    u = _unlisted_in_mask(c)
    print("tetras: %d selected rays, unlisted boxes in the mask:" % len(u), np.bincount(u))
    assert (u >= 2).sum() >= 1000 and (u >= 3).sum() >= 100


def test_panes_walks_in_full_beside_clipped_rays_and_resolves_on_specular_boxes(zoo_cases):
    """measured: 486 of 4 247 path-like rays hit two or more listed boxes (a full walk, selector 0) and 698
    are selected; 451 and 622 path-like direct rays on the glass and the mirror pane"""
    c = zoo_cases("panes")
    n = c["n_path"]
    two = c["lst"][:n].sum(axis=1) >= 2
    print("panes: %d path-like rays, %d through two or more listed boxes, %d selected" %
          (n, two.sum(), c["sel"][:n].sum()))
    assert two.sum() >= 100 and not (two & c["sel"][:n]).any() and c["sel"][:n].any()
    for group in ("glass", "mirror"):
        k, hits = _direct_on(c, group)
        print("panes: %d path-like direct rays on %s, %d hit it" % (k, group, hits))
        assert k >= 50


def test_many_clips_over_merged_boxes_and_keeps_direct_rays(zoo_cases):
    """measured: 6 819 + 327 selected rays with 2 / 3 unlisted boxes in their mask, 503 path-like direct rays"""
    c = zoo_cases("many")
    u = _unlisted_in_mask(c)
    nd = int(c["direct"][: c["n_path"]].sum())
    print("many: %d selected rays, unlisted boxes in the mask:" % len(u), np.bincount(u), "; %d path-like direct rays" % nd)
    assert (u >= 2).sum() >= 1000 and nd >= 100
