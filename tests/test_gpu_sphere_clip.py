"""The wavefront's sphere clip on the GPU (render_launch.hpp "Sphere clip"): in a
lean render of a scene in LDS whose clip walk is active, the secondary extends are
wf_sphere_clip, which cuts each unlisted box of a clipped ray's selector to the
sphere over that box's triangles before it takes the union; a ray with nothing left
starts no walk.  Which rays are culled, direct, clipped or walked does not change,
and the image stays the oracle's bit for bit.

Every case asserts lean = counting = oracle bit for bit with equal `rays`, and that
a second lean render repeats the first, counters included.  `extend_rays`,
`direct_rays` and `clipped_rays` are the values tests/golden/shade_carry_counters.json
holds for the same render (recorded before the clip walk's extend knew spheres).

`sphere_skips` (the selected rays whose walk a sphere left nothing of): equal, with
`clipped_rays`, to what the C restatement of the start-up (scripts/price_sphere_clip.c,
on the CPU oracle, which makes the same rays) counts for the same frame; between 0 and
`clipped_rays`, exclusive, on scene01 at depth >= 2; 0 for counting renders, wf_sort =
1, the global layout, QuinEngine, the megakernel, scenes without
boxes and a scene whose unlisted box gets no sphere.

Hand-made scenes: `ball` -- a UV sphere of 96 triangles in front of a two-triangle
wall under a two-triangle light: the clustering spends its six other boxes on the
ball (two caps, four side pieces), each with a sphere of its own, so a selector names
several unlisted boxes whose spheres overlap, and the rays through their corners skip
their walk; `ribbon` -- the same with a flat strip in place of the ball, whose
vertices reach its box's corners: no sphere, so the plain extend runs.
"""
import json
import math
import os

import numpy as np
import pytest

from test_direct_lists import LIGHT, MTL, dl_scenes  # noqa: F401  (dl_scenes: a fixture)
from test_direct_resolve import FRAMES, _params
from test_miss_cull import INSIDE, _same
from test_primary_lists import CAMERAS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_carry_counters.json")
KEYS = ("rays", "extend_rays", "direct_rays", "clipped_rays")
FRAMES = dict(FRAMES, c=(48, 48, 5, 2))
HAND_CAM = dict(eye=(0.0, 4.0, 9.0), direction=(0.0, -0.1, -1.0))
WALL = "v -6 0 -6\nv 6 0 -6\nv 6 8 -6\nv -6 8 -6\n"


def _ball_obj(slices=8, stacks=7, centre=(0.0, 3.0, 0.0), radius=2.0):
    """a UV sphere: 2 * slices * (stacks - 1) triangles, poles on the y axis"""
    v = [(centre[0], centre[1] + radius, centre[2])]
    for i in range(1, stacks):
        th = math.pi * i / stacks
        for j in range(slices):
            ph = 2.0 * math.pi * j / slices
            v.append((centre[0] + radius * math.sin(th) * math.cos(ph), centre[1] + radius * math.cos(th),
                      centre[2] + radius * math.sin(th) * math.sin(ph)))
    v.append((centre[0], centre[1] - radius, centre[2]))
    ring = lambda i, j: 2 + (i - 1) * slices + j % slices  # noqa: E731  (1-based .obj index)
    f = []
    for j in range(slices):
        f.append((1, ring(1, j + 1), ring(1, j)))
        f.append((len(v), ring(stacks - 1, j), ring(stacks - 1, j + 1)))
        for i in range(1, stacks - 1):
            f.append((ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i + 1, j)))
    return v, f


def _hand_obj(name, verts, faces):
    n0 = len(verts)
    s = "mtllib %s.mtl\n" % name + "".join("v %.9g %.9g %.9g\n" % p for p in verts) + WALL + LIGHT
    s += "vn 0 1 0\nvn 0 0 1\nvn 0 -1 0\ng thing\nusemtl grey\n"
    s += "".join("f %d//1 %d//1 %d//1\n" % t for t in faces)
    s += "g wall\nusemtl red\nf %d//2 %d//2 %d//2 %d//2\n" % tuple(n0 + i for i in (1, 2, 3, 4))
    s += "g light\nusemtl glow\nf %d//3 %d//3 %d//3 %d//3\n" % tuple(n0 + i for i in (5, 6, 7, 8))
    return s


def _ribbon():
    """a flat strip of 12 triangles in the plane y = 1, corners at its box's corners"""
    v, f = [], []
    for i in range(7):
        x = -5.0 + 10.0 * i / 6
        v += [(x, 1.0, -1.0), (x, 1.0, 1.0)]
    for i in range(6):
        a = 2 * i + 1
        f += [(a, a + 1, a + 3), (a, a + 3, a + 2)]
    return v, f


@pytest.fixture(scope="session")
def sc_scenes(mcpt, dl_scenes, tmp_path_factory):  # noqa: F811
    paths = dict(dl_scenes, scene02=mcpt.scene_path("scene02"), scene03=mcpt.scene_path("scene03"))
    for name, (v, f) in {"ball": _ball_obj(), "ribbon": _ribbon()}.items():
        d = tmp_path_factory.mktemp("sc_" + name)
        (d / (name + ".obj")).write_text(_hand_obj(name, v, f))
        (d / (name + ".mtl")).write_text(MTL)
        paths[name] = str(d / (name + ".obj"))
    return paths


@pytest.fixture(scope="session")
def sc_oracle(oracle_mod, sc_scenes):
    """(scene, frame, depth, camera, mode) -> the oracle's (image, counters), rendered once and read-only"""
    have, scenes = {}, {}

    def get(name, frame, depth, cam=None, qe=False):
        key = (name, frame, depth, tuple(sorted((cam or {}).items())), qe)
        if key not in have:
            if name not in scenes:
                scenes[name] = oracle_mod.Scene(sc_scenes[name])
            w, h, spp, chunk = FRAMES[frame]
            kw = dict(cam or {})
            if qe:
                kw.update(mode=oracle_mod.MODE_QE, seed=0x5EED, illum=1.0, fov=45.0, fresnel_kd=0)
            img, cnt = scenes[name].render(oracle_mod.RenderParams(
                width=w, height=h, spp=spp, spp_chunk=chunk, max_depth=depth, threads=16, **kw))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    return get


@pytest.fixture(scope="session")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# the frames whose sphere_skips the C restatement (scripts/price_sphere_clip.c) gives: scene, frame, depth, camera
PRICED = [("scene01", f, d, None) for f in ("a", "b") for d in (1, 2, 7)] + [
    ("scene01", "a", 3, "near_sphere"), ("scene01", "a", 3, "inside"), ("scene01", "g4", 7, "INSIDE"),
    ("ball", "a", 1, "HAND"), ("ball", "a", 3, "HAND"), ("ribbon", "a", 3, "HAND")]


def _cam(name):
    return None if name is None else INSIDE if name == "INSIDE" else HAND_CAM if name == "HAND" else CAMERAS[name]


@pytest.fixture(scope="session")
def priced(sc_scenes, tmp_path_factory):
    """(scene, frame, depth, camera) -> the restatement's accumulators for that frame on the CPU oracle, which
    makes the same rays: "sel" is the device's clipped_rays, "skips" its sphere_skips.  One child process for
    all frames: the restatement is the oracle compiled with hooks, a second copy of its library"""
    import subprocess
    import sys
    cases = []
    for name, frame, depth, cam in PRICED:
        w, h, spp, chunk = FRAMES[frame]
        cases.append(dict(path=sc_scenes[name], width=w, height=h, spp=spp, chunk=chunk, max_depth=depth,
                          cam=_cam(cam)))
    f = tmp_path_factory.mktemp("sc_priced") / "cases.json"
    f.write_text(json.dumps(cases))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "price_sphere_clip.py"), "--cases", str(f)],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    return dict(zip(PRICED, json.loads(out.strip().splitlines()[-1])))


def _priced_equal(priced, key, ls):
    acc = priced[key]
    assert acc["clip_diff"] == 0 and acc["sph_diff"] == 0, (key, acc)
    assert (int(ls["clipped_rays"]), int(ls["sphere_skips"])) == (acc["sel"], acc["skips"]), (key, ls, acc)


def _p(mcpt, frame, depth, **kw):
    w, h, spp, chunk = FRAMES[frame]
    return mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=chunk, tile=kw.pop("tile", 8), max_depth=depth,
                             pipeline="wavefront", wf_sort=kw.pop("sort", False), lean=kw.pop("lean", True),
                             **(kw.pop("cam", None) or {}), **kw)


def _check(mcpt, scene, ref, rc, frame, depth, cam=None, **kw):
    """lean = counting = oracle, bits and rays; a second lean render repeats the first; -> the lean stats"""
    lean, ls = scene.render(_p(mcpt, frame, depth, cam=cam, **kw))
    full, fs = scene.render(_p(mcpt, frame, depth, lean=False, cam=cam, **kw))
    again, as_ = scene.render(_p(mcpt, frame, depth, cam=cam, **kw))
    print("depth %d: rays %d, extend %d, direct %d, clipped %d, sphere skips %d" % (
        depth, ls["rays"], ls["extend_rays"], ls["direct_rays"], ls["clipped_rays"], ls["sphere_skips"]))
    assert _same(lean, ref) and _same(full, ref) and _same(again, lean)
    assert ls["rays"] == rc["rays"] and fs["rays"] == rc["rays"]
    assert ls["paths"] == rc["paths"] and ls["shades"] == rc["shades"]
    assert fs["sphere_skips"] == 0 and fs["clipped_rays"] == 0 and fs["extend_rays"] == rc["rays"] - rc["paths"]
    assert {k: as_[k] for k in KEYS + ("sphere_skips",)} == {k: ls[k] for k in KEYS + ("sphere_skips",)}
    assert 0 <= ls["sphere_skips"] <= ls["clipped_rays"] <= ls["extend_rays"]
    return ls


# ---- without a GPU ---------------------------------------------------------------------------

def test_hand_made_scenes_are_what_they_say(mcpt, sc_scenes):
    from montecarlopathtracer_amd._capi import lib
    ball = mcpt.Scene(mcpt.ObjModel(sc_scenes["ball"]), host_only=True)
    dl = ball.direct_lists()
    # the clustering spends its whole box budget: two caps and four side pieces, each with a sphere
    assert sorted(dl["box_tris"]) == [2, 2, 12, 12, 12, 12, 24, 24] and sorted(dl["counts"]) == [0] * 6 + [2, 2]
    cs = ball.clip_spheres()
    assert cs["mask"] == sum(1 << int(b) for b in np.flatnonzero(dl["counts"] == 0))
    boxes = ball.miss_cull_boxes()
    for b in np.flatnonzero(dl["counts"] == 0):
        assert np.array_equal(cs["spheres"][b, :3], (boxes[b, :3] + boxes[b, 3:]) * np.float32(0.5))
        assert 0.0 < cs["spheres"][b, 3] < float(((boxes[b, 3:] - boxes[b, :3]) ** 2).sum()) / 4
    assert not cs["spheres"][dl["counts"] > 0].any()
    ribbon = mcpt.Scene(mcpt.ObjModel(sc_scenes["ribbon"]), host_only=True)
    assert sorted(ribbon.direct_lists()["box_tris"]) == [2, 2, 12] and ribbon.clip_spheres()["mask"] == 0
    assert int(lib().mcpt_scene_sphere_skips(ball.handle)) == 0 and int(lib().mcpt_scene_sphere_skips(None)) == 0
    assert int(lib().mcpt_scene_clip_spheres(None, None)) == 0


# ---- on the GPU ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 7])
@pytest.mark.parametrize("frame", ["a", "b"])
def test_scene01_matches_oracle_and_keeps_its_counters(mcpt, sc_oracle, sc_scenes, golden, priced, frame, depth):
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    assert bin(scene.clip_spheres()["mask"]).count("1") == 2
    ref, rc = sc_oracle("scene01", frame, depth)
    ls = _check(mcpt, scene, ref, rc, frame, depth)
    assert {k: int(ls[k]) for k in KEYS} == golden["scene01-%s-d%d" % (frame, depth)]
    _priced_equal(priced, ("scene01", frame, depth, None), ls)
    if depth >= 2:
        assert 0 < ls["sphere_skips"] < ls["clipped_rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("cam", ["near_sphere", "inside"])
def test_cameras_near_and_inside(mcpt, sc_oracle, sc_scenes, priced, cam):
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    ref, rc = sc_oracle("scene01", "a", 3, cam=CAMERAS[cam])
    ls = _check(mcpt, scene, ref, rc, "a", 3, cam=CAMERAS[cam])
    _priced_equal(priced, ("scene01", "a", 3, cam), ls)
    assert 0 < ls["sphere_skips"] < ls["clipped_rays"]


@pytest.mark.gpu
def test_camera_inside_looking_out_keeps_its_counters(mcpt, sc_oracle, sc_scenes, golden, priced):
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    ref, rc = sc_oracle("scene01", "g4", 7, cam=INSIDE)
    ls = _check(mcpt, scene, ref, rc, "g4", 7, cam=INSIDE)
    assert {k: int(ls[k]) for k in KEYS} == golden["inside-g4"]
    _priced_equal(priced, ("scene01", "g4", 7, "INSIDE"), ls)


@pytest.mark.gpu
def test_scene02(mcpt, sc_oracle, sc_scenes):
    """scene02's image is read from global memory: no lists, no selectors, the plain extend"""
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene02"]))
    ref, rc = sc_oracle("scene02", "c", 3)
    ls = _check(mcpt, scene, ref, rc, "c", 3)
    assert ls["sphere_skips"] == 0 and ls["clipped_rays"] == 0


@pytest.mark.gpu
def test_tile_4(mcpt, sc_oracle, sc_scenes, golden, priced):
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    ref, rc = sc_oracle("scene01", "b", 7)
    ls = _check(mcpt, scene, ref, rc, "b", 7, tile=4)
    assert {k: int(ls[k]) for k in KEYS} == golden["tile4"] and 0 < ls["sphere_skips"] < ls["clipped_rays"]
    _priced_equal(priced, ("scene01", "b", 7, None), ls)                     # (the frame's rays, whatever the tile)


@pytest.mark.gpu
def test_two_packed_shards_sum_to_the_frames_counters(mcpt, sc_oracle, sc_scenes, golden, priced):
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    w, h = FRAMES["b"][:2]
    got = np.full((h, w, 3), -1.0, np.float32)
    tot = dict.fromkeys(KEYS + ("sphere_skips",), 0)
    for r in range(2):
        p = _params(mcpt, "b", 7, shard_count=2, shard_index=r)
        part, st = scene.render(p)
        for k in tot:
            tot[k] += int(st[k])
        xy = p.shard_pixels()
        ok = xy[:, 0] >= 0
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
    ref, rc = sc_oracle("scene01", "b", 7)
    assert _same(got, ref) and tot["rays"] == rc["rays"]
    assert {k: tot[k] for k in KEYS} == golden["shards"]
    # what becomes of a ray depends on the ray alone: the shards' skips are the whole frame's
    _, whole = scene.render(_params(mcpt, "b", 7))
    assert tot["sphere_skips"] == whole["sphere_skips"] > 0
    _priced_equal(priced, ("scene01", "b", 7, None), tot)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_ball_in_front_of_a_wall(mcpt, sc_oracle, sc_scenes, priced, depth):
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["ball"]))
    assert not scene.info()["node_boxes"] and scene.clip_spheres()["mask"] != 0
    ref, rc = sc_oracle("ball", "a", depth, cam=HAND_CAM)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    ls = _check(mcpt, scene, ref, rc, "a", depth, cam=HAND_CAM)
    _priced_equal(priced, ("ball", "a", depth, "HAND"), ls)
    if depth == 3:
        assert 0 < ls["sphere_skips"] < ls["clipped_rays"]


@pytest.mark.gpu
def test_thin_mesh_gets_no_sphere_and_skips_nothing(mcpt, sc_oracle, sc_scenes, priced):
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["ribbon"]))
    assert scene.clip_spheres()["mask"] == 0
    ref, rc = sc_oracle("ribbon", "a", 3, cam=HAND_CAM)
    ls = _check(mcpt, scene, ref, rc, "a", 3, cam=HAND_CAM)
    _priced_equal(priced, ("ribbon", "a", 3, "HAND"), ls)
    assert ls["clipped_rays"] > 0 and ls["sphere_skips"] == 0


@pytest.mark.gpu
def test_renders_that_do_not_clip_to_spheres_skip_nothing(mcpt, sc_oracle, sc_scenes):
    ref, rc = sc_oracle("scene01", "a", 2)
    w, h, spp, chunk = FRAMES["a"]
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    img, st = scene.render(_p(mcpt, "a", 2, sort=True))                       # wf_sort = 1: the plain extend
    assert _same(img, ref) and st["clipped_rays"] > 0 and st["sphere_skips"] == 0
    img, st = scene.render(mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=chunk, max_depth=2, lean=True))
    assert _same(img, ref) and st["rays"] == rc["rays"] and st["sphere_skips"] == 0     # the megakernel
    glob = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]), layout="global")
    img, st = glob.render(_p(mcpt, "a", 2))
    assert _same(img, ref) and st["sphere_skips"] == 0 and st["clipped_rays"] == 0
    room = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene03"]))
    assert room.info()["miss_cull_boxes"] == 0 and room.clip_spheres()["mask"] == 0
    rref, _ = sc_oracle("scene03", "a", 2)
    img, st = room.render(_p(mcpt, "a", 2))
    assert _same(img, rref) and st["sphere_skips"] == 0


@pytest.mark.gpu
def test_quinengine(mcpt, sc_oracle, sc_scenes, golden):
    depth = 2
    ref, rc = sc_oracle("scene01", "a", depth, qe=True)
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    w, h, spp, chunk = FRAMES["a"]
    for lean in (True, False):
        img, st = scene.render(mcpt.RenderParams.for_quinengine(
            width=w, height=h, spp=spp, spp_chunk=chunk, tile=8, max_depth=depth, seed=0x5EED, pipeline="wavefront",
            lean=lean))
        assert _same(img, ref) and st["rays"] == rc["rays"], lean
        # QuinEngine keeps the plain extend, lean or counting
        assert st["sphere_skips"] == 0
        if lean:
            assert {k: int(st[k]) for k in KEYS} == golden["qe-lean"]


@pytest.mark.gpu
def test_replays_of_a_captured_lean_render_keep_counting(mcpt, sc_oracle, sc_scenes):
    """a lean render captured into a graph issues wf_sphere_clip once, at capture; every replay runs it, and the
    record read afterwards holds the replays' skips beside their clipped rays -- twice one render's for two
    replays -- and the next record none"""
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(sc_scenes["scene01"]))
    p = _p(mcpt, "a", 7)
    ref, rc = sc_oracle("scene01", "a", 7)
    img, one = scene.render(p)
    assert _same(img, ref) and 0 < one["sphere_skips"] < one["clipped_rays"]
    scene.reserve(p)
    w, h = FRAMES["a"][:2]
    fb = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        scene.render_device(p, fb.data_ptr(), s.cuda_stream)
    for _ in range(2):
        fb.zero_()
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(fb.view(h, w, 4)[..., :3].cpu().numpy(), ref)
    two = scene.stats()
    for k in KEYS + ("sphere_skips",):
        assert two[k] == 2 * one[k], (k, two[k], one[k])
    none = scene.stats()
    assert none["sphere_skips"] == 0 and none["clipped_rays"] == 0 and none["rays"] == 0
