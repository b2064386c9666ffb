"""Primary rays resolved from per-tile candidate lists (render_launch.hpp
"Primary lists"): lean wavefront renders of a scene in LDS list, per 8x8
tile, the triangles the tile's jitter-grown frustum can touch, and bounce 0
tests those instead of walking the KD tree.  The closest hit is the minimum of
(t, rank) over the triangles tested, so the image and the ray count stay the
oracle's bit for bit -- checked here for every case, together with the
counting render of the same frame, which still walks.

Frames are scene01, at most 64 x 64 px and 3 spp.  Cameras:

* default      eye (0, 5, 17): tiles beside the box (no candidate), wall tiles
               (two), sphere silhouettes and interiors (more than K)
* inside       eye inside the box: no tile without a candidate
* near_sphere  a short distance from the glass sphere: nearly every list is
               longer than K, the walk fallback runs
* diagonal     rolled so that the back wall's diagonal (-5.76, 10, -5) --
               (5.76, 0, -5) projects onto the image's middle row boundary, a
               tile edge: both wall triangles meet on tile edges
* graze        eye at the root box's top right edge (x = max, y = max), looking
               along it: the middle rays graze two root box faces
"""
import os

import numpy as np
import pytest

DEPTH = 3
CAMERAS = {
    "default": dict(eye=(0.0, 5.0, 17.0)),
    "inside": dict(eye=(0.0, 5.0, 4.0)),
    "near_sphere": dict(eye=(2.3, 1.8, 5.0)),
    "diagonal": dict(eye=(0.0, 5.0, 17.0), up=(0.6552717017267126, 0.7553932730149099, 0.0)),
    "graze": dict(eye=(5.7639699, 10.0, 17.0)),
}


@pytest.fixture(scope="session")
def lists_oracle(oracle_mod, mcpt):
    """(camera, width, height, spp, chunk[, QE]) -> the oracle's (image, counters), rendered once, read-only"""
    have = {}
    scene = []

    def get(cam, w, h, spp, chunk, qe=False):
        key = (cam, w, h, spp, chunk, qe)
        if key not in have:
            if not scene:
                scene.append(oracle_mod.Scene(mcpt.scene_path("scene01")))
            kw = dict(CAMERAS[cam])
            if qe:
                kw.update(mode=oracle_mod.MODE_QE, seed=0x5EED, illum=1.0, fov=45.0, fresnel_kd=0)
            img, cnt = scene[0].render(oracle_mod.RenderParams(
                width=w, height=h, spp=spp, spp_chunk=chunk, max_depth=2 if qe else DEPTH,
                threads=min(os.cpu_count() or 8, 16), **kw))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    return get


def _params(mcpt, cam, w, h, spp, chunk, lean=True, **kw):
    return mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=chunk, max_depth=DEPTH, pipeline="wavefront",
                             lean=lean, **CAMERAS[cam], **kw)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check(mcpt, scene, lists_oracle, cam, w, h, spp, chunk, **kw):
    """lean == oracle == counting, bit for bit, with equal ray counts; returns the lean render's tile classes"""
    ref, rc = lists_oracle(cam, w, h, spp, chunk)
    lean, ls = scene.render(_params(mcpt, cam, w, h, spp, chunk, **kw))
    cls = scene.primary_tile_classes()
    full, fs = scene.render(_params(mcpt, cam, w, h, spp, chunk, lean=False, **kw))
    assert scene.primary_tile_classes() == {"empty": 0, "listed": 0, "walked": 0, "k": cls["k"]}   # counting walks
    assert _same(lean, ref) and _same(full, ref)
    assert ls["rays"] == rc["rays"] and ls["paths"] == rc["paths"]
    assert fs["rays"] == rc["rays"] and fs["tri_tests"] == rc["tri_tests"]
    return cls


# ---- without a GPU ---------------------------------------------------------------------------

def test_no_render_no_classes(mcpt):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    cls = scene.primary_tile_classes()
    assert cls["k"] >= 1 and (cls["empty"], cls["listed"], cls["walked"]) == (0, 0, 0)


# ---- on the GPU ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene01(mcpt):
    return mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))


@pytest.mark.gpu
def test_default_camera_uses_all_three_classes(mcpt, scene01, lists_oracle):
    """64 x 64, 2 spp: tiles without a candidate, listed tiles and walked tiles
    all occur; were they all zero, the render fell back to the walk silently."""
    cls = _check(mcpt, scene01, lists_oracle, "default", 64, 64, 2, 2)
    assert cls["empty"] + cls["listed"] + cls["walked"] == 64
    assert cls["empty"] > 0 and cls["listed"] > 0 and cls["walked"] > 0, cls   # (so for K = 4 and for K = 8)


@pytest.mark.gpu
def test_odd_width_and_chunks(mcpt, scene01, lists_oracle):
    """48 x 64 (width no power of two: the mapping divides) and 64 x 48, 3 spp in chunks of 2"""
    cls = _check(mcpt, scene01, lists_oracle, "default", 48, 64, 3, 2)
    assert cls["empty"] + cls["listed"] + cls["walked"] == 6 * 8
    cls = _check(mcpt, scene01, lists_oracle, "default", 64, 48, 3, 2)
    assert cls["empty"] + cls["listed"] + cls["walked"] == 8 * 6


@pytest.mark.gpu
@pytest.mark.parametrize("cam", ["inside", "near_sphere", "diagonal", "graze"])
def test_cameras(mcpt, scene01, lists_oracle, cam):
    cls = _check(mcpt, scene01, lists_oracle, cam, 64, 64, 2, 2)
    assert cls["empty"] + cls["listed"] + cls["walked"] == 64
    if cam == "inside":
        assert cls["empty"] == 0 and cls["listed"] > 0
    if cam == "near_sphere":
        assert cls["walked"] > 32, cls                      # the walk fallback carries the frame
    if cam == "graze":
        assert cls["empty"] > 0 and cls["listed"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [8, 4])
def test_small_frame_and_other_tile(mcpt, scene01, lists_oracle, tile):
    """24 x 24: nine 8x8 tiles use the lists; 4x4 tiles keep the walk (a 64-slot
    group is then four tiles) and report no list use"""
    cls = _check(mcpt, scene01, lists_oracle, "default", 24, 24, 2, 2, tile=tile)
    if tile == 8:
        assert cls["empty"] + cls["listed"] + cls["walked"] == 9 and cls["listed"] + cls["walked"] > 0
    else:
        assert (cls["empty"], cls["listed"], cls["walked"]) == (0, 0, 0)


@pytest.mark.gpu
def test_two_packed_shards_reassemble(mcpt, scene01, lists_oracle):
    ref, rc = lists_oracle("default", 64, 48, 3, 2)
    got = np.full((48, 64, 3), -1.0, np.float32)
    rays = 0
    for r in range(2):
        p = _params(mcpt, "default", 64, 48, 3, 2, shard_count=2, shard_index=r)
        part, st = scene01.render(p)
        cls = scene01.primary_tile_classes()
        assert cls["empty"] + cls["listed"] + cls["walked"] == 24 and cls["listed"] > 0
        rays += st["rays"]
        xy = p.shard_pixels()
        ok = xy[:, 0] >= 0
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
    assert _same(got, ref) and rays == rc["rays"]


@pytest.mark.gpu
def test_quinengine_lean_unchanged(mcpt, scene01, lists_oracle):
    ref, rc = lists_oracle("default", 64, 48, 2, 2, qe=True)
    img, st = scene01.render(mcpt.RenderParams.for_quinengine(
        width=64, height=48, spp=2, spp_chunk=2, max_depth=2, seed=0x5EED, pipeline="wavefront", lean=True))
    cls = scene01.primary_tile_classes()
    assert (cls["empty"], cls["listed"], cls["walked"]) == (0, 0, 0)
    assert _same(img, ref) and st["rays"] == rc["rays"]


@pytest.mark.gpu
def test_global_layout_unchanged(mcpt, lists_oracle):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), layout="global")
    assert scene.info()["node_boxes"] == 1
    ref, rc = lists_oracle("default", 64, 64, 2, 2)
    img, st = scene.render(_params(mcpt, "default", 64, 64, 2, 2))
    cls = scene.primary_tile_classes()
    assert (cls["empty"], cls["listed"], cls["walked"]) == (0, 0, 0)
    assert _same(img, ref) and st["rays"] == rc["rays"]
