"""The wavefront's direct lists on the GPU (render_launch.hpp "Direct lists"):
in lean renders of a scene in LDS the shade marks a new ray whose segment hits
exactly one occluder box, a small one, and the extend resolves it from that
box's triangles without a tree walk.  The image stays the oracle's bit for bit.

The oracle (which walks every ray) is the reference everywhere: every lean
render must give its image and its `rays`, and the counting render (lists off,
`direct_rays == 0`) the same.  Frames are 64 x 64 or 48 x 64 px, 5 spp in
chunks of 2.  Scenes other than scene01 (closed and lone are
tests/test_miss_cull.py's):

* closed      scene01 with a front wall: no occluder boxes, so no lists
* lone        one emitting triangle: no boxes either
* kquads      a diffuse back wall of exactly K = 2 triangles (listed), a diffuse
              floor of K + 1 (a fan of three: walked) and a two-triangle light
              over them; the floor's rays towards the wall are direct, the wall's
              towards the floor walk
* seam        a floor and a back wall of two triangles each, meeting at the edge
              y = 0, z = -6, seen from a grazing camera that looks along that
              edge, with a light above: the primary hits crowd the seam, and the
              rays that leave them start a hair off one box and run close to the
              other (a ray that hits both boxes is walked; rays lying exactly in
              a box plane cannot be placed by a render,
              tests/test_direct_lists_cpu.py holds them)
"""
import os

import numpy as np
import pytest

from test_miss_cull import INSIDE, LONE_MTL, LONE_OBJ, _same

CHUNK = 2
FRAMES = {"a": (64, 64, 5), "b": (48, 64, 5)}       # width, height, spp
DEPTHS = (0, 1, 2, 7)

MTL = ("newmtl grey\nKd 0.7 0.7 0.7\nKa 0 0 0\nnewmtl red\nKd 0.7 0.3 0.3\nKa 0 0 0\n"
       "newmtl glow\nKd 0.5 0.5 0.5\nKa 0.6 0.5 0.4\n")
LIGHT = """v -2 8 -4
v 2 8 -4
v 2 8 0
v -2 8 0
"""
KQUADS_OBJ = """mtllib kquads.mtl
v -6 0 -6
v 6 0 -6
v 6 0 6
v 0 0 6
v -6 0 6
v -6 0 -6
v 6 0 -6
v 6 8 -6
v -6 8 -6
""" + LIGHT + """vn 0 1 0
vn 0 0 1
vn 0 -1 0
g floor
usemtl grey
f 1//1 3//1 2//1
f 1//1 4//1 3//1
f 1//1 5//1 4//1
g wall
usemtl red
f 6//2 7//2 8//2 9//2
g light
usemtl glow
f 10//3 11//3 12//3 13//3
"""
SEAM_OBJ = """mtllib seam.mtl
v -6 0 -6
v 6 0 -6
v 6 0 6
v -6 0 6
v -6 0 -6
v 6 0 -6
v 6 8 -6
v -6 8 -6
""" + LIGHT + """vn 0 1 0
vn 0 0 1
vn 0 -1 0
g floor
usemtl grey
f 1//1 4//1 3//1 2//1
g wall
usemtl red
f 5//2 6//2 7//2 8//2
g light
usemtl glow
f 9//3 10//3 11//3 12//3
"""
KQUADS_CAM = dict(eye=(0.0, 5.0, 7.0), direction=(0.0, -0.3, -1.0))
SEAM_CAM = dict(eye=(-6.5, 1.0, -5.0), direction=(1.0, -0.1, -0.1))     # along the seam, just off both quads


@pytest.fixture(scope="session")
def dl_scenes(mcpt, tmp_path_factory):
    """name -> .obj path"""
    src = mcpt.scene_path("scene01")
    obj = open(src).read()
    mtl = open(os.path.splitext(src)[0] + ".mtl").read()
    closed = obj + "g pFront\nusemtl initialShadingGroup\nf 1/1/1 2/2/1 4/4/1 3/3/1\n"
    paths = {"scene01": src}
    for name, (o, m, mname) in {"closed": (closed, mtl, "scene01.mtl"), "lone": (LONE_OBJ, LONE_MTL, "lone.mtl"),
                                "kquads": (KQUADS_OBJ, MTL, "kquads.mtl"), "seam": (SEAM_OBJ, MTL, "seam.mtl")}.items():
        d = tmp_path_factory.mktemp("dl_" + name)
        (d / (name + ".obj")).write_text(o)
        (d / mname).write_text(m)
        paths[name] = str(d / (name + ".obj"))
    return paths


@pytest.fixture(scope="session")
def dl_oracle(oracle_mod, dl_scenes):
    """(scene, frame, depth, camera, mode) -> the oracle's (image, counters), rendered once and read-only"""
    have, scenes = {}, {}

    def get(name, frame, depth, cam=None, qe=False):
        key = (name, frame, depth, tuple(sorted((cam or {}).items())), qe)
        if key not in have:
            if name not in scenes:
                scenes[name] = oracle_mod.Scene(dl_scenes[name])
            w, h, spp = FRAMES[frame]
            kw = dict(cam or {})
            if qe:
                kw.update(mode=oracle_mod.MODE_QE, seed=0x5EED, illum=1.0, fov=45.0, fresnel_kd=0)
            img, cnt = scenes[name].render(oracle_mod.RenderParams(
                width=w, height=h, spp=spp, spp_chunk=CHUNK, max_depth=depth, threads=min(os.cpu_count() or 8, 16),
                **kw))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    return get


def _params(mcpt, frame, depth, lean=True, sort=False, cam=None, **kw):
    w, h, spp = FRAMES[frame]
    return mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=kw.pop("tile", 8), max_depth=depth,
                             pipeline="wavefront", wf_sort=sort, lean=lean, **(cam or {}), **kw)


def _check(mcpt, scene, ref, rc, frame, depth, sort=False, cam=None, **kw):
    """lean (lists on where the scene has them) = counting (lists off) = oracle: image bits and
    ray count; -> the lean render's direct rays"""
    lean, ls = scene.render(_params(mcpt, frame, depth, sort=sort, cam=cam, **kw))
    full, fs = scene.render(_params(mcpt, frame, depth, lean=False, sort=sort, cam=cam, **kw))
    assert _same(lean, ref) and _same(full, ref)
    assert ls["rays"] == rc["rays"] and fs["rays"] == rc["rays"]
    assert ls["paths"] == rc["paths"] and ls["shades"] == rc["shades"]
    assert fs["direct_rays"] == 0
    assert 0 <= ls["direct_rays"] <= ls["rays"] - ls["paths"]
    return ls["direct_rays"]


# ---- without a GPU: what the hand-made scenes are ---------------------------------------------

def test_hand_made_scenes_have_the_lists_they_are_for(mcpt, dl_scenes):
    k = mcpt.Scene(mcpt.ObjModel(dl_scenes["kquads"]), host_only=True)
    dl = k.direct_lists()
    assert dl["k"] == 2 and sorted(dl["box_tris"]) == [2, 2, 3]
    assert sorted(dl["counts"]) == [0, 2, 2]                   # the floor's K + 1 triangles keep the walk
    floor = k.miss_cull_boxes()[np.flatnonzero(dl["counts"] == 0)[0]]
    assert floor[1] == floor[4] == 0.0
    flat = k.miss_cull_boxes()
    assert ((flat[:, 3:] - flat[:, :3]) == 0).any(axis=1).all()
    s = mcpt.Scene(mcpt.ObjModel(dl_scenes["seam"]), host_only=True)
    assert sorted(s.direct_lists()["counts"]) == [2, 2, 2]
    b = s.miss_cull_boxes()
    floor, wall = b[b[:, 4] == 0][0], b[(b[:, 2] == -6) & (b[:, 5] == -6)][0]
    assert floor[2] == wall[2] == -6 and floor[1] == wall[1] == 0   # they share the edge y = 0, z = -6
    for name in ("closed", "lone"):
        c = mcpt.Scene(mcpt.ObjModel(dl_scenes[name]), host_only=True)
        assert c.info()["miss_cull_boxes"] == 0 and c.info()["direct_list_boxes"] == 0


# ---- on the GPU ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_scene01_matches_oracle(mcpt, dl_oracle, dl_scenes, frame, depth, sort):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    assert scene.info()["direct_list_boxes"] == 5
    ref, rc = dl_oracle("scene01", frame, depth)
    direct = _check(mcpt, scene, ref, rc, frame, depth, sort=sort)
    if depth >= 1:
        assert direct > 0
        if depth == 7:                                             # (priced: two thirds of the walked rays)
            assert direct > 0.3 * (rc["rays"] - rc["paths"])
    else:
        assert direct == 0                                         # depth 0's only secondary rays ... are none


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_tile_4(mcpt, dl_oracle, dl_scenes, sort):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    ref, rc = dl_oracle("scene01", "b", 7)
    assert _check(mcpt, scene, ref, rc, "b", 7, sort=sort, tile=4) > 0


@pytest.mark.gpu
def test_two_packed_shards_reassemble(mcpt, dl_oracle, dl_scenes):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    w, h, _ = FRAMES["b"]
    got = np.full((h, w, 3), -1.0, np.float32)
    rays = direct = 0
    for r in range(2):
        p = _params(mcpt, "b", 7, shard_count=2, shard_index=r)
        part, st = scene.render(p)
        rays += st["rays"]
        direct += st["direct_rays"]
        assert st["direct_rays"] > 0
        xy = p.shard_pixels()
        ok = xy[:, 0] >= 0
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
    ref, rc = dl_oracle("scene01", "b", 7)
    assert _same(got, ref) and rays == rc["rays"]
    # the shards' direct rays are the whole frame's: the selector depends on the ray alone
    assert direct == scene.render(_params(mcpt, "b", 7))[1]["direct_rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_quinengine_lean(mcpt, dl_oracle, dl_scenes, sort):
    depth = 2
    ref, rc = dl_oracle("scene01", "a", depth, qe=True)
    assert float(ref.max()) > 0.0
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    w, h, spp = FRAMES["a"]
    for lean in (True, False):
        img, st = scene.render(mcpt.RenderParams.for_quinengine(
            width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=depth, seed=0x5EED, pipeline="wavefront",
            wf_sort=sort, lean=lean))
        assert _same(img, ref) and st["rays"] == rc["rays"], lean
        assert (st["direct_rays"] > 0) == lean


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 7])
def test_global_layout_keeps_the_walk(mcpt, dl_oracle, dl_scenes, depth):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]), layout="global")
    assert scene.info()["node_boxes"] == 1 and scene.info()["miss_cull_boxes"] == 8
    ref, rc = dl_oracle("scene01", "a", depth)
    assert _check(mcpt, scene, ref, rc, "a", depth) == 0


@pytest.mark.gpu
def test_megakernel_reports_no_direct_rays(mcpt, dl_oracle, dl_scenes):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    w, h, spp = FRAMES["a"]
    ref, rc = dl_oracle("scene01", "a", 2)
    img, st = scene.render(mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=CHUNK, max_depth=2, lean=True))
    assert _same(img, ref) and st["rays"] == rc["rays"] and st["direct_rays"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_camera_inside_looking_out(mcpt, dl_oracle, dl_scenes, sort):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    ref, rc = dl_oracle("scene01", "a", 7, cam=INSIDE)
    assert _check(mcpt, scene, ref, rc, "a", 7, sort=sort, cam=INSIDE) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,cam", [("closed", dict(eye=(0.0, 5.0, 4.0))),
                                      ("lone", dict(eye=(0.0, 4.0, 9.0)))])
def test_scene_without_boxes(mcpt, dl_oracle, dl_scenes, name, cam):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes[name]))
    assert scene.info()["miss_cull_boxes"] == 0
    ref, rc = dl_oracle(name, "a", 2, cam=cam)
    assert float(ref.max()) > 0.0
    assert _check(mcpt, scene, ref, rc, "a", 2, cam=cam) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", [1, 3])
def test_quad_of_k_is_listed_and_of_k_plus_1_walked(mcpt, dl_oracle, dl_scenes, depth, sort):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["kquads"]))
    assert sorted(scene.direct_lists()["counts"]) == [0, 2, 2]
    ref, rc = dl_oracle("kquads", "a", depth, cam=KQUADS_CAM)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    assert _check(mcpt, scene, ref, rc, "a", depth, sort=sort, cam=KQUADS_CAM) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", [1, 3])
def test_rays_along_a_seam(mcpt, dl_oracle, dl_scenes, depth, sort):
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["seam"]))
    ref, rc = dl_oracle("seam", "b", depth, cam=SEAM_CAM)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    direct = _check(mcpt, scene, ref, rc, "b", depth, sort=sort, cam=SEAM_CAM)
    assert 0 < direct < rc["rays"] - rc["paths"]
