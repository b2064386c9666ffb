"""The wavefront's clip walk on the GPU (render_launch.hpp "Clip walk"): in
lean renders where the direct lists are active, a walking ray through at least
one occluder box without a list and at most one with a list carries its box mask;
the lean LDS extend walks it only inside its unlisted boxes' slab interval, its
listed box's two triangles tested first.  The image stays the oracle's bit for bit.

The oracle (which walks every ray in full) is the reference everywhere: every
lean render must give its image and its `rays`, and the counting render (no
culls, no lists, no selectors) the same.  Frames are 64 x 64 or 48 x 64 px, 5 spp
in chunks of 2, and one 256 x 256 frame whose segments span several blocks.

Counter (`scene.render(...)[1]["clipped_rays"]`): the rays an extend started
with a selector.  They are among `extend_rays` (the rays the secondary extends
took), so 0 < clipped_rays <= extend_rays on a lean LDS render of depth >= 1 of
a scene with an unlisted box; 0 for counting renders, the global layout, the
megakernel and scene03 (a closed room: no boxes).

Scenes beside scene01 and scene02: test_direct_lists.py's kquads, whose floor of
K + 1 triangles is the smallest box without a list (the wall's rays towards it
are clipped, and most have the listed light or wall in their mask as well).
"""
import numpy as np
import pytest

from test_direct_lists import KQUADS_CAM, dl_scenes  # noqa: F401  (dl_scenes: a fixture)
from test_miss_cull import INSIDE, _same

CHUNK = 2
FRAMES = {"a": (64, 64, 5), "b": (48, 64, 5), "big": (256, 256, 5)}       # width, height, spp
DEPTHS = (0, 1, 2, 7)


@pytest.fixture(scope="module")
def cw_scenes(mcpt, dl_scenes):  # noqa: F811
    return dict(dl_scenes, scene02=mcpt.scene_path("scene02"), scene03=mcpt.scene_path("scene03"))


@pytest.fixture(scope="module")
def cw_oracle(oracle_mod, cw_scenes):
    """(scene, frame, depth, camera, mode) -> the oracle's (image, counters), rendered once and read-only"""
    have, scenes = {}, {}

    def get(name, frame, depth, cam=None, qe=False):
        key = (name, frame, depth, tuple(sorted((cam or {}).items())), qe)
        if key not in have:
            if name not in scenes:
                scenes[name] = oracle_mod.Scene(cw_scenes[name])
            w, h, spp = FRAMES[frame]
            kw = dict(cam or {})
            if qe:
                kw.update(mode=oracle_mod.MODE_QE, seed=0x5EED, illum=1.0, fov=45.0, fresnel_kd=0)
            img, cnt = scenes[name].render(oracle_mod.RenderParams(
                width=w, height=h, spp=spp, spp_chunk=CHUNK, max_depth=depth, threads=16, **kw))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    return get


def _params(mcpt, frame, depth, lean=True, sort=False, cam=None, **kw):
    w, h, spp = FRAMES[frame]
    return mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=depth,
                             pipeline="wavefront", wf_sort=sort, lean=lean, **(cam or {}), **kw)


def _check(mcpt, scene, ref, rc, frame, depth, sort=False, cam=None, clipped=None):
    """lean = counting = oracle: image bits and ray count; the counting render clips nothing, the lean
    one's clipped rays are among its extends' (clipped: whether it must have some); -> the lean stats"""
    lean, ls = scene.render(_params(mcpt, frame, depth, sort=sort, cam=cam))
    full, fs = scene.render(_params(mcpt, frame, depth, lean=False, sort=sort, cam=cam))
    print("depth %d: rays %d, extend %d, direct %d, clipped %d" % (depth, ls["rays"], ls["extend_rays"],
                                                                  ls["direct_rays"], ls["clipped_rays"]))
    assert _same(lean, ref) and _same(full, ref)
    assert ls["rays"] == rc["rays"] and fs["rays"] == rc["rays"]
    assert ls["paths"] == rc["paths"] and ls["shades"] == rc["shades"]
    assert fs["clipped_rays"] == 0 and fs["extend_rays"] == rc["rays"] - rc["paths"]
    assert 0 <= ls["clipped_rays"] <= ls["extend_rays"]
    if clipped is not None:
        assert (ls["clipped_rays"] > 0) == clipped
    return ls


# ---- without a GPU ---------------------------------------------------------------------------

def test_stats_report_clipped_rays(mcpt, dl_scenes):  # noqa: F811
    """the C accessor exists and a scene that has not rendered reports none"""
    s = mcpt.Scene(mcpt.ObjModel(dl_scenes["kquads"]), host_only=True)
    from montecarlopathtracer_amd._capi import lib
    assert int(lib().mcpt_scene_clipped_rays(s.handle)) == 0 and int(lib().mcpt_scene_clipped_rays(None)) == 0


# ---- on the GPU ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("frame", ["a", "b"])
@pytest.mark.parametrize("name", ["scene01", "scene02"])
def test_matches_oracle(mcpt, cw_oracle, cw_scenes, name, frame, depth, sort):
    """scene02 keeps the full walk (global layout: no lists); depth 0 has no secondary ray; depth 1's only
    secondary extend is the terminal query's, behind the terminal cull (which keeps a ray's selector with it)"""
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes[name]))
    assert scene.info()["direct_list_boxes"] > 0 and (scene.direct_lists()["counts"] == 0).any()
    in_lds = not scene.info()["node_boxes"]                    # (scene02's image is read from global memory)
    assert in_lds == (name == "scene01")
    ref, rc = cw_oracle(name, frame, depth)
    _check(mcpt, scene, ref, rc, frame, depth, sort=sort, clipped=in_lds and depth >= 1)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_camera_inside_the_box(mcpt, cw_oracle, cw_scenes, sort):
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene01"]))
    ref, rc = cw_oracle("scene01", "a", 7, cam=INSIDE)
    _check(mcpt, scene, ref, rc, "a", 7, sort=sort, cam=INSIDE, clipped=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("which", [0, 1])
def test_eye_inside_an_object_box(mcpt, cw_oracle, cw_scenes, which, sort):
    """the eye at the centre of one of scene01's two large boxes: the first hits are inside the object, so
    the rays that leave them start inside their unlisted box and its slab interval begins at 0"""
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene01"]))
    boxes, tris = scene.miss_cull_boxes(), scene.direct_lists()["box_tris"]
    b = boxes[np.argsort(tris)[::-1][which]]
    assert tris.max() > 100
    cam = dict(eye=tuple(float(x) for x in (b[:3] + b[3:]) / 2), direction=(0.3, -0.2, -1.0))
    ref, rc = cw_oracle("scene01", "a", 3, cam=cam)
    assert rc["shades"] > 0
    _check(mcpt, scene, ref, rc, "a", 3, sort=sort, cam=cam, clipped=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_quinengine(mcpt, cw_oracle, cw_scenes, sort):
    depth = 2
    ref, rc = cw_oracle("scene01", "a", depth, qe=True)
    assert float(ref.max()) > 0.0
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene01"]))
    w, h, spp = FRAMES["a"]
    for lean in (True, False):
        img, st = scene.render(mcpt.RenderParams.for_quinengine(
            width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=depth, seed=0x5EED, pipeline="wavefront",
            wf_sort=sort, lean=lean))
        assert _same(img, ref) and st["rays"] == rc["rays"], lean
        assert (st["clipped_rays"] > 0) == lean and st["clipped_rays"] <= st["extend_rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", [1, 3])
def test_box_of_k_plus_1_is_clipped(mcpt, cw_oracle, cw_scenes, depth, sort):
    """kquads: the floor's fan of K + 1 triangles is the smallest box without a list"""
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes["kquads"]))
    assert sorted(scene.direct_lists()["counts"]) == [0, 2, 2]
    ref, rc = cw_oracle("kquads", "a", depth, cam=KQUADS_CAM)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    _check(mcpt, scene, ref, rc, "a", depth, sort=sort, cam=KQUADS_CAM, clipped=True if depth == 3 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_segments_of_several_blocks(mcpt, cw_oracle, cw_scenes, sort):
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene01"]))
    ref, rc = cw_oracle("scene01", "big", 2)
    ls = _check(mcpt, scene, ref, rc, "big", 2, sort=sort, clipped=True)
    assert ls["clipped_rays"] > 0.1 * ls["extend_rays"]          # (priced: 97% of the walked rays)


@pytest.mark.gpu
def test_global_layout_and_scene_without_boxes_clip_nothing(mcpt, cw_oracle, cw_scenes):
    glob = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene01"]), layout="global")
    ref, rc = cw_oracle("scene01", "a", 2)
    _check(mcpt, glob, ref, rc, "a", 2, clipped=False)
    room = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene03"]))
    assert room.info()["miss_cull_boxes"] == 0
    ref, rc = cw_oracle("scene03", "a", 2)
    _check(mcpt, room, ref, rc, "a", 2, clipped=False)


@pytest.mark.gpu
def test_megakernel_clips_nothing(mcpt, cw_oracle, cw_scenes):
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene01"]))
    w, h, spp = FRAMES["a"]
    ref, rc = cw_oracle("scene01", "a", 2)
    img, st = scene.render(mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=CHUNK, max_depth=2, lean=True))
    assert _same(img, ref) and st["rays"] == rc["rays"] and st["clipped_rays"] == 0


@pytest.mark.gpu
def test_two_renders_are_bit_identical(mcpt, cw_scenes):
    """queue order depends on scheduling; nothing reads it, and what becomes of a ray depends on the ray alone"""
    scene = mcpt.Scene(mcpt.ObjModel(cw_scenes["scene01"]))
    a, sa = scene.render(_params(mcpt, "a", 7))
    b, sb = scene.render(_params(mcpt, "a", 7))
    assert _same(a, b)
    keys = ("rays", "direct_rays", "extend_rays", "clipped_rays")
    assert {k: sa[k] for k in keys} == {k: sb[k] for k in keys}
