"""The wavefront's miss cull (render_launch.hpp "Miss cull"): in lean renders
the shade that creates a ray ends the path at once when the ray misses every
occluder box of the scene, and the image stays the oracle's bit for bit.

The oracle (which walks every ray) is the reference everywhere; every lean
render must give its image and its `rays`, and the counting render (cull off)
the same.  Frames are 64 x 64 or 48 x 64 px, 5-8 spp in odd chunks.  Scenes
other than scene01:

* closed      scene01 with a front wall over its opening: every face of the
              scene bounds is a flat box, so the scene gets no boxes
* lone        one tilted emitting triangle: its only box spans the scene
              bounds (a degenerate box set), no boxes either
* quads       a diffuse floor quad and an emitting quad standing on it in the
              plane x = 0, which also holds the eye: primary rays graze the
              standing quad's zero-thickness box and the floor's secondary rays
              start a hair off the floor's (rays lying exactly in a box plane
              cannot be placed by a render; tests/test_miss_cull_cpu.py holds them)
"""
import os

import numpy as np
import pytest

CHUNK = 3
FRAMES = {"a": (64, 64, 6), "b": (48, 64, 7)}       # width, height, spp
DEPTHS = (0, 1, 2, 7)
INSIDE = dict(eye=(0.5, 5.0, 4.0), direction=(1.0, -0.2, 0.45))   # inside the box, looking out past the right wall's edge

LONE_OBJ = """mtllib lone.mtl
v -3 1 -2
v 4 2 -1
v 0 8 -4
vn 0 0 1
g tri
usemtl glow
f 1//1 2//1 3//1
"""
LONE_MTL = "newmtl glow\nKd 0.5 0.5 0.5\nKa 0.6 0.5 0.4\n"
QUADS_OBJ = """mtllib quads.mtl
v -6 0 -6
v 6 0 -6
v 6 0 6
v -6 0 6
v 0 0 -3
v 0 0 1
v 0 4 1
v 0 4 -3
vn 0 1 0
vn 1 0 0
g floor
usemtl grey
f 1//1 4//1 3//1 2//1
g fin
usemtl glow
f 5//2 6//2 7//2 8//2
"""
QUADS_MTL = "newmtl grey\nKd 0.7 0.7 0.7\nKa 0 0 0\nnewmtl glow\nKd 0.5 0.5 0.5\nKa 0.6 0.5 0.4\n"


@pytest.fixture(scope="session")
def miss_scenes(mcpt, tmp_path_factory):
    """name -> .obj path"""
    src = mcpt.scene_path("scene01")
    obj = open(src).read()
    mtl = open(os.path.splitext(src)[0] + ".mtl").read()
    # (vertices 1-4 of scene01 are the corners of its opening, z = 5)
    closed = obj + "g pFront\nusemtl initialShadingGroup\nf 1/1/1 2/2/1 4/4/1 3/3/1\n"
    paths = {"scene01": src}
    for name, (o, m, mname) in {"closed": (closed, mtl, "scene01.mtl"), "lone": (LONE_OBJ, LONE_MTL, "lone.mtl"),
                                "quads": (QUADS_OBJ, QUADS_MTL, "quads.mtl")}.items():
        d = tmp_path_factory.mktemp("miss_" + name)
        (d / (name + ".obj")).write_text(o)
        (d / mname).write_text(m)
        paths[name] = str(d / (name + ".obj"))
    return paths


@pytest.fixture(scope="session")
def oracle_frame(oracle_mod, miss_scenes):
    """(scene, frame, depth, camera, mode) -> the oracle's (image, counters), rendered once and read-only"""
    have, scenes = {}, {}

    def get(name, frame, depth, cam=None, qe=False):
        key = (name, frame, depth, tuple(sorted((cam or {}).items())), qe)
        if key not in have:
            if name not in scenes:
                scenes[name] = oracle_mod.Scene(miss_scenes[name])
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


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check(mcpt, scene, ref, rc, frame, depth, sort=False, cam=None, **kw):
    """lean (cull on) = counting (cull off) = oracle: image bits and ray count"""
    lean, ls = scene.render(_params(mcpt, frame, depth, sort=sort, cam=cam, **kw))
    full, fs = scene.render(_params(mcpt, frame, depth, lean=False, sort=sort, cam=cam, **kw))
    assert _same(lean, ref) and _same(full, ref)
    assert ls["rays"] == rc["rays"] and fs["rays"] == rc["rays"]
    assert ls["paths"] == rc["paths"] and ls["shades"] == rc["shades"]


# ---- without a GPU: what the frames exercise ------------------------------------------------

def test_frames_hold_escaping_and_kept_rays(oracle_frame):
    """Oracle counters only.  scene01 from the C2 camera: the paths that end on
    the light at depth 1 make lit pixels that do not see it directly (kept
    secondary rays), and a deeper render ends paths early -- fewer rays than
    max_depth + 2 per path (rays that left through the opening or hit the light)."""
    mask0 = oracle_frame("scene01", "a", 0)[0].any(axis=2)
    lit1 = oracle_frame("scene01", "a", 1)[0].any(axis=2)
    assert mask0.any() and (lit1 & ~mask0).any()
    rc = oracle_frame("scene01", "a", 7)[1]
    assert rc["rays"] < 0.8 * 8 * rc["paths"]
    # the camera inside the box: most paths end with their second ray (it leaves through the opening)
    ri = oracle_frame("scene01", "a", 7, cam=INSIDE)[1]
    assert ri["shades"] > 0.5 * ri["paths"] and ri["rays"] < 3.0 * ri["paths"]


# ---- on the GPU ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_scene01_matches_oracle(mcpt, oracle_frame, miss_scenes, frame, depth, sort):
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes["scene01"]))
    n = scene.info()["miss_cull_boxes"]
    assert 5 <= n <= 16 and scene.miss_cull_boxes().shape == (n, 6)
    ref, rc = oracle_frame("scene01", frame, depth)
    _check(mcpt, scene, ref, rc, frame, depth, sort=sort)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_tile_4(mcpt, oracle_frame, miss_scenes, sort):
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes["scene01"]))
    ref, rc = oracle_frame("scene01", "b", 7)
    _check(mcpt, scene, ref, rc, "b", 7, sort=sort, tile=4)


@pytest.mark.gpu
def test_two_packed_shards_reassemble(mcpt, oracle_frame, miss_scenes):
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes["scene01"]))
    w, h, _ = FRAMES["b"]
    got = np.full((h, w, 3), -1.0, np.float32)
    rays = 0
    for r in range(2):
        p = _params(mcpt, "b", 7, shard_count=2, shard_index=r)
        part, st = scene.render(p)
        rays += st["rays"]
        xy = p.shard_pixels()
        ok = xy[:, 0] >= 0
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
    ref, rc = oracle_frame("scene01", "b", 7)
    assert _same(got, ref) and rays == rc["rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 7])
def test_global_layout(mcpt, oracle_frame, miss_scenes, depth):
    """the same shade in front of the global-memory extend"""
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes["scene01"]), layout="global")
    assert scene.info()["miss_cull_boxes"] >= 5 and scene.info()["node_boxes"] == 1
    ref, rc = oracle_frame("scene01", "a", depth)
    _check(mcpt, scene, ref, rc, "a", depth)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_quinengine_lean(mcpt, oracle_frame, miss_scenes, sort):
    """QuinEngine mode: a miss ends the path with zero at every bounce, roulette or not"""
    depth = 2
    ref, rc = oracle_frame("scene01", "a", depth, qe=True)
    assert float(ref.max()) > 0.0
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes["scene01"]))
    w, h, spp = FRAMES["a"]
    for lean in (True, False):
        img, st = scene.render(mcpt.RenderParams.for_quinengine(
            width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=depth, seed=0x5EED, pipeline="wavefront",
            wf_sort=sort, lean=lean))
        assert _same(img, ref) and st["rays"] == rc["rays"], lean


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_camera_inside_looking_out(mcpt, oracle_frame, miss_scenes, sort):
    """nearly every secondary ray leaves through the opening and is culled"""
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes["scene01"]))
    ref, rc = oracle_frame("scene01", "a", 7, cam=INSIDE)
    _check(mcpt, scene, ref, rc, "a", 7, sort=sort, cam=INSIDE)


@pytest.mark.gpu
@pytest.mark.parametrize("name,cam", [("closed", dict(eye=(0.0, 5.0, 4.0))),
                                      ("lone", dict(eye=(0.0, 4.0, 9.0)))])
def test_scene_without_boxes(mcpt, oracle_frame, miss_scenes, name, cam):
    """closed: a room nothing can leave; lone: a box set that is the scene bounds.
    No boxes, no cull, the oracle's image."""
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes[name]))
    assert scene.info()["miss_cull_boxes"] == 0 and scene.miss_cull_boxes().shape == (0, 6)
    ref, rc = oracle_frame(name, "a", 2, cam=cam)
    assert float(ref.max()) > 0.0
    _check(mcpt, scene, ref, rc, "a", 2, cam=cam)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_quads_rays_along_a_box_plane(mcpt, oracle_frame, miss_scenes, depth):
    cam = dict(eye=(0.0, 1.5, 9.0))
    scene = mcpt.Scene(mcpt.ObjModel(miss_scenes["quads"]))
    boxes = scene.miss_cull_boxes()
    assert scene.info()["miss_cull_boxes"] == 2
    assert sorted((b[3:] - b[:3] == 0).argmax() for b in boxes) == [0, 1]      # flat in x, flat in y
    ref, rc = oracle_frame("quads", "b", depth, cam=cam)
    assert float(ref.max()) > 0.0
    for sort in (False, True):
        _check(mcpt, scene, ref, rc, "b", depth, sort=sort, cam=cam)
