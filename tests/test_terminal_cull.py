"""The wavefront's terminal cull (render_launch.hpp "Terminal cull"): lean
renders drop the rays of the path loop's last query that can reach no emitter
box, and the image stays the oracle's bit for bit.

The oracle (which walks every ray) is the reference everywhere.  Frames are
64 x 48 px, 8 spp, tile 8; scenes other than scene01 are scene01 with its .mtl
(and, for more than 8 emitters, its groups) edited:

* flat        initialShadingGroup (three wall faces) emits too: many terminal
              hits, rays grazing the emitters' planes
* flat_sides  the two side walls emit: emitter boxes of zero thickness
* negative    a non-emitter with Ka -0.5 0 0: the terminal query adds negative
              radiance, so the scene must not be culled
* many        the mirror sphere cut into 9 emitting geometries: 10 emitters,
              more than the 8 boxes a scene may have
"""
import os
import re

import numpy as np
import pytest

W, H, SPP, CHUNK, TILE = 64, 48, 8, 4, 8
DEPTHS = (0, 1, 2, 7)


def _edit_mtl(text, material, line):
    """the .mtl text with `material`'s Ka (or Kd, by the line's key) replaced by `line`"""
    key = line.split()[0]
    out, cur, done = [], None, False
    for l in text.splitlines():
        if l.startswith("newmtl"):
            cur = l.split()[1]
        if cur == material and l.split()[:1] == [key]:
            l, done = line, True
        out.append(l)
    assert done, (material, key)
    return "\n".join(out) + "\n"


def _split_group(obj_text, group, parts):
    """the .obj text with the faces of `group` dealt to `parts` consecutive groups"""
    lines = obj_text.splitlines()
    at = lines.index("g " + group)
    faces = [i for i in range(at, len(lines)) if lines[i].startswith("f ")]
    end = next((i for i in range(at + 1, len(lines)) if lines[i].startswith("g ")), len(lines))
    faces = [i for i in faces if i < end]
    per = (len(faces) + parts - 1) // parts
    assert len(faces) >= parts
    for k in range(parts - 1, 0, -1):               # (back to front: the indices before stay valid)
        lines.insert(faces[k * per], "g %s_%02d" % (group, k))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="session")
def cull_scenes(mcpt, tmp_path_factory):
    """name -> .obj path"""
    src = mcpt.scene_path("scene01")
    obj = open(src).read()
    mtl = open(os.path.splitext(src)[0] + ".mtl").read()
    assert re.search(r"^mtllib scene01.mtl$", obj, re.M)
    variants = {
        "flat": (obj, _edit_mtl(mtl, "initialShadingGroup", "Ka 0.30 0.20 0.10")),
        "flat_sides": (obj, _edit_mtl(_edit_mtl(mtl, "lambert2SG", "Ka 0.25 0.00 0.00"),
                                      "lambert3SG", "Ka 0.00 0.00 0.25")),
        "negative": (obj, _edit_mtl(mtl, "lambert2SG", "Ka -0.5 0 0")),
        "many": (_split_group(obj, "pSphere1", 9), _edit_mtl(mtl, "sphere_mirror", "Ka 0.10 0.10 0.10")),
        "nan_kd": (obj, _edit_mtl(mtl, "lambert3SG", "Kd nan 0 1")),
    }
    paths = {"scene01": src}
    for name, (o, m) in variants.items():
        d = tmp_path_factory.mktemp("cull_" + name)
        (d / "scene01.obj").write_text(o)
        (d / "scene01.mtl").write_text(m)
        paths[name] = str(d / "scene01.obj")
    return paths


@pytest.fixture(scope="session")
def oracle_frame(oracle_mod, cull_scenes):
    """(name, max_depth[, spp]) -> the oracle's (image, counters), rendered once and read-only"""
    have, scenes = {}, {}

    def get(name, depth, spp=SPP, mode=None, **kw):
        key = (name, depth, spp, mode)
        if key not in have:
            if name not in scenes:
                scenes[name] = oracle_mod.Scene(cull_scenes[name])
            if mode is not None:
                kw["mode"] = mode
            img, cnt = scenes[name].render(oracle_mod.RenderParams(
                width=W, height=H, spp=spp, spp_chunk=CHUNK, max_depth=depth, threads=min(os.cpu_count() or 8, 16),
                **kw))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    return get


def _params(mcpt, depth, lean=True, sort=False, **kw):
    return mcpt.RenderParams(width=W, height=H, spp=SPP, spp_chunk=CHUNK, tile=TILE, max_depth=depth,
                             pipeline="wavefront", wf_sort=sort, lean=lean, **kw)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- without a GPU: the host's decision, and what the frames exercise ----------------------

@pytest.mark.parametrize("name,boxes", [("scene01", 1), ("flat", 2), ("flat_sides", 3), ("negative", 0), ("many", 0),
                                        ("nan_kd", 0)])
def test_scene_qualification(mcpt, cull_scenes, name, boxes):
    """One box per emitter geometry when every non-emitter has Ka == 0, every Kd
    and Ks is finite and there are 1..8 emitters; else none, in either layout."""
    for layout in ("auto", "global"):
        scene = mcpt.Scene(mcpt.ObjModel(cull_scenes[name]), layout=layout, host_only=True)
        assert scene.info()["terminal_cull_boxes"] == boxes, (name, layout)
    if name == "many":                              # the case is what it says: more than 8 emitter geometries
        geoms = scene.kd()[3]
        assert int((geoms[:, 0:3] > 0).any(axis=1).sum()) == 10


def test_no_emitter_no_cull(mcpt, cull_scenes, tmp_path):
    src = cull_scenes["scene01"]
    (tmp_path / "scene01.obj").write_text(open(src).read())
    (tmp_path / "scene01.mtl").write_text(_edit_mtl(open(os.path.splitext(src)[0] + ".mtl").read(),
                                                    "blinn2SG", "Ka 0 0 0"))
    scene = mcpt.Scene(mcpt.ObjModel(str(tmp_path / "scene01.obj")), host_only=True)
    assert scene.info()["terminal_cull_boxes"] == 0


def test_frames_hold_kept_terminal_rays(oracle_frame):
    """Oracle images only: at max_depth 1 some pixel that does not see the light
    directly is lit, so a terminal ray that passes the box test (and reaches
    the emitter) is part of the frames the GPU tests compare."""
    mask0 = oracle_frame("scene01", 0)[0].any(axis=2)
    lit1 = oracle_frame("scene01", 1)[0].any(axis=2)
    assert mask0.any() and (lit1 & ~mask0).any()


# ---- on the GPU ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_scene01_lean_matches_oracle(mcpt, oracle_frame, cull_scenes, depth, sort):
    scene = mcpt.Scene(mcpt.ObjModel(cull_scenes["scene01"]))
    assert scene.info()["terminal_cull_boxes"] == 1
    ref, rc = oracle_frame("scene01", depth)
    img, st = scene.render(_params(mcpt, depth, sort=sort))
    assert _same(img, ref)
    assert st["rays"] == rc["rays"] and st["paths"] == rc["paths"] and st["shades"] == rc["shades"]


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_lean_equals_counting_render(mcpt, oracle_frame, cull_scenes, depth, sort):
    """The counting render walks every ray (the cull is off) and keeps the
    oracle's visit counters; the lean render gives its image and ray count."""
    scene = mcpt.Scene(mcpt.ObjModel(cull_scenes["scene01"]))
    full, fs = scene.render(_params(mcpt, depth, lean=False, sort=sort))
    lean, ls = scene.render(_params(mcpt, depth, lean=True, sort=sort))
    assert _same(lean, full) and ls["rays"] == fs["rays"]
    rc = oracle_frame("scene01", depth)[1]
    for k in ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades"):
        assert fs[k] == rc[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat", "flat_sides"])
@pytest.mark.parametrize("depth", [1, 7])
def test_flat_emitters_match_oracle(mcpt, oracle_frame, cull_scenes, name, depth):
    scene = mcpt.Scene(mcpt.ObjModel(cull_scenes[name]))
    assert scene.info()["terminal_cull_boxes"] == (2 if name == "flat" else 3)
    ref, rc = oracle_frame(name, depth)
    for sort in (False, True):
        img, st = scene.render(_params(mcpt, depth, sort=sort))
        assert _same(img, ref), sort
        assert st["rays"] == rc["rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["negative", "many"])
@pytest.mark.parametrize("depth", [1, 7])
def test_scene_without_cull_matches_oracle(mcpt, oracle_frame, cull_scenes, name, depth):
    """negative: the terminal query collects negative radiance from a
    non-emitter; many: more emitter geometries than boxes.  No cull, oracle's image."""
    scene = mcpt.Scene(mcpt.ObjModel(cull_scenes[name]))
    assert scene.info()["terminal_cull_boxes"] == 0
    ref, rc = oracle_frame(name, depth)
    if name == "negative":
        assert float(ref.min()) < 0.0
    img, st = scene.render(_params(mcpt, depth))
    assert _same(img, ref) and st["rays"] == rc["rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 7])
def test_global_layout_lean_matches_oracle(mcpt, oracle_frame, cull_scenes, depth):
    """the same cull in front of the global-memory extend"""
    scene = mcpt.Scene(mcpt.ObjModel(cull_scenes["scene01"]), layout="global")
    assert scene.info()["terminal_cull_boxes"] == 1 and scene.info()["node_boxes"] == 1
    ref, rc = oracle_frame("scene01", depth)
    img, st = scene.render(_params(mcpt, depth))
    assert _same(img, ref) and st["rays"] == rc["rays"]


@pytest.mark.gpu
def test_two_packed_shards_reassemble(mcpt, oracle_frame, cull_scenes):
    scene = mcpt.Scene(mcpt.ObjModel(cull_scenes["scene01"]))
    full, _ = scene.render(_params(mcpt, 7))
    got = np.full((H, W, 3), -1.0, np.float32)
    for r in range(2):
        p = _params(mcpt, 7, shard_count=2, shard_index=r)
        part, _ = scene.render(p)
        xy = p.shard_pixels()
        ok = xy[:, 0] >= 0
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
    assert _same(got, full) and _same(full, oracle_frame("scene01", 7)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_quinengine_lean_matches_oracle(mcpt, oracle_mod, oracle_frame, cull_scenes, sort):
    """QuinEngine mode: the query at depth 3 * max_depth is never read, so lean
    renders drop all of its rays; image and ray count stay the oracle's."""
    depth, seed = 2, 0x5EED
    ref, rc = oracle_frame("scene01", depth, mode=oracle_mod.MODE_QE, seed=seed, illum=1.0, fov=45.0, fresnel_kd=0)
    scene = mcpt.Scene(mcpt.ObjModel(cull_scenes["scene01"]))
    img, st = scene.render(mcpt.RenderParams.for_quinengine(
        width=W, height=H, spp=SPP, spp_chunk=CHUNK, tile=TILE, max_depth=depth, seed=seed, pipeline="wavefront",
        wf_sort=sort, lean=True))
    assert float(ref.max()) > 0.0
    assert _same(img, ref) and st["rays"] == rc["rays"]
