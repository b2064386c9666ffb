"""The queue-order shade's terminal cull and carry on the GPU (render_launch.hpp
"Terminal cull", "Direct resolve"): in a lean render of a scene in LDS with
occluder boxes the shade that makes the terminal query's ray also tests it
against the emitter boxes -- no wf_cull_terminal runs -- and a lane whose new
ray it resolved keeps that ray and shades it in the wave's next iteration
instead of writing it to the next queue's tail and reading it back.  Queues
then hold rays of mixed depths, and waves take their slots from a counter.

Nothing the caller sees may change: every case asserts lean = counting =
oracle bit for bit with equal `rays`, and that two renders of the frame agree.
Which rays are walked, direct or clipped is a property of each ray, not of the
schedule, and the rays the terminal cull drops never reached an extend before
either: `extend_rays`, `direct_rays` and `clipped_rays` must be the values the
commit before the carry reported for the same render, recorded on the GPU in
tests/golden/shade_carry_counters.json (scripts/record_shade_carry_counters.py).

Cases (mirroring test_direct_resolve.py): scene01 at 64 x 64 and 48 x 64, 5 spp
in chunks of 2, depths 0, 1, 2, 7 -- at depth 1 the terminal cull sits in the
first resolving shade, at depth 2 a carried ray's product is the terminal ray;
a camera inside the box with whole 64-slot groups per segment (waves run out of
slots while lanes still carry); 256 x 256 (several blocks per segment); tile 4;
two packed shards; QuinEngine; scenes without boxes (nothing carried); the
hand-made wall of K and floor of K + 1 triangles and the seam.  wf_sort = 1, the
global layout and the megakernel must be unaffected.
"""
import json
import os

import numpy as np
import pytest

from test_direct_lists import KQUADS_CAM, SEAM_CAM, dl_scenes  # noqa: F401  (dl_scenes: a fixture)
from test_direct_resolve import FRAMES, _params, dr_oracle  # noqa: F401  (dr_oracle: a fixture)
from test_miss_cull import INSIDE, _same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_carry_counters.json")
KEYS = ("rays", "extend_rays", "direct_rays", "clipped_rays")
# case id -> the counters its lean render reported (the recording script reads this)
SEEN = {}

CLOSED_CAM = dict(eye=(0.0, 5.0, 4.0))
LONE_CAM = dict(eye=(0.0, 4.0, 9.0))
# id -> (scene, frame, depth, camera, render keywords)
CASES = {}
for _f in ("a", "b"):
    for _d in (0, 1, 2, 7):
        CASES["scene01-%s-d%d" % (_f, _d)] = ("scene01", _f, _d, None, {})
for _f in ("g1", "g4", "g16"):
    CASES["inside-%s" % _f] = ("scene01", _f, 7, INSIDE, {})
CASES["big"] = ("scene01", "big", 2, None, {})
CASES["tile4"] = ("scene01", "b", 7, None, dict(tile=4))
CASES["closed"] = ("closed", "a", 2, CLOSED_CAM, {})
CASES["lone"] = ("lone", "a", 2, LONE_CAM, {})
for _d in (1, 3):
    CASES["kquads-d%d" % _d] = ("kquads", "a", _d, KQUADS_CAM, {})
    CASES["seam-d%d" % _d] = ("seam", "b", _d, SEAM_CAM, {})
# unaffected configurations: the sorting shade (no carry, the cull kernel) and the global layout
CASES["sorted-d2"] = ("scene01", "a", 2, None, dict(sort=True))
CASES["sorted-d7"] = ("scene01", "b", 7, None, dict(sort=True))
CASES["global-d1"] = ("scene01", "a", 1, None, dict(layout="global"))
CASES["global-d7"] = ("scene01", "a", 7, None, dict(layout="global"))


@pytest.fixture(scope="session")
def golden():
    if not os.path.exists(GOLDEN):                   # (recording: every comparison then fails, after SEEN is filled)
        return {}
    with open(GOLDEN) as f:
        return json.load(f)


def _counters(st):
    return {k: int(st[k]) for k in KEYS}


def _pin(golden, cid, st):
    """the lean render's counters are the parent commit's for this render"""
    SEEN[cid] = _counters(st)
    assert SEEN[cid] == golden[cid], (cid, SEEN[cid], golden[cid])


# ---- without a GPU ---------------------------------------------------------------------------

def test_fixture_covers_every_case(golden):
    want = set(CASES) | {"shards", "qe-lean"}
    assert set(golden) == want, sorted(set(golden) ^ want)
    for cid, g in golden.items():
        assert set(g) == set(KEYS), cid
    # the cases are what they say: rays resolved (so carried) below the terminal depth, terminal
    # rays culled, and nothing of either where the scene has no boxes
    assert golden["scene01-a-d7"]["direct_rays"] > 0 and golden["scene01-a-d7"]["clipped_rays"] > 0
    assert golden["scene01-a-d0"]["direct_rays"] == 0 and golden["scene01-a-d0"]["extend_rays"] == 0
    assert golden["closed"]["direct_rays"] == 0 and golden["lone"]["direct_rays"] == 0
    assert golden["global-d7"]["direct_rays"] == 0 and golden["sorted-d7"]["direct_rays"] > 0


# ---- on the GPU ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_case_matches_oracle_and_parent_counters(mcpt, dr_oracle, dl_scenes, golden, cid):  # noqa: F811
    name, frame, depth, cam, kw = CASES[cid]
    kw = dict(kw)
    layout = kw.pop("layout", None)
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes[name]), **({"layout": layout} if layout else {}))
    ref, rc = dr_oracle(name, frame, depth, cam=cam)
    lean, ls = scene.render(_params(mcpt, frame, depth, cam=cam, **kw))
    full, fs = scene.render(_params(mcpt, frame, depth, lean=False, cam=cam, **kw))
    again, as_ = scene.render(_params(mcpt, frame, depth, cam=cam, **kw))
    assert _same(lean, ref) and _same(full, ref) and _same(again, lean)
    assert ls["rays"] == rc["rays"] and fs["rays"] == rc["rays"]
    assert ls["paths"] == rc["paths"] and ls["shades"] == rc["shades"]
    assert fs["direct_rays"] == 0 and fs["extend_rays"] == rc["rays"] - rc["paths"]
    assert _counters(as_) == _counters(ls)
    _pin(golden, cid, ls)


@pytest.mark.gpu
def test_two_packed_shards_sum_to_the_parent_counters(mcpt, dr_oracle, dl_scenes, golden):  # noqa: F811
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    w, h = FRAMES["b"][:2]
    got = np.full((h, w, 3), -1.0, np.float32)
    tot = dict.fromkeys(KEYS, 0)
    for r in range(2):
        p = _params(mcpt, "b", 7, shard_count=2, shard_index=r)
        part, st = scene.render(p)
        for k in KEYS:
            tot[k] += int(st[k])
        xy = p.shard_pixels()
        ok = xy[:, 0] >= 0
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
    ref, rc = dr_oracle("scene01", "b", 7)
    assert _same(got, ref) and tot["rays"] == rc["rays"]
    _pin(golden, "shards", tot)
    # what becomes of a ray depends on the ray alone: the shards' counters are the whole frame's
    assert tot == golden["scene01-b-d7"]


@pytest.mark.gpu
def test_quinengine_lean_and_counting(mcpt, dr_oracle, dl_scenes, golden):  # noqa: F811
    """QuinEngine: every ray of the query at depth 3 * max_depth is dropped where it is made"""
    depth = 2
    ref, rc = dr_oracle("scene01", "a", depth, qe=True)
    assert float(ref.max()) > 0.0
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    w, h, spp, chunk = FRAMES["a"]
    out = {}
    for lean in (True, False, True):
        img, st = scene.render(mcpt.RenderParams.for_quinengine(
            width=w, height=h, spp=spp, spp_chunk=chunk, tile=8, max_depth=depth, seed=0x5EED, pipeline="wavefront",
            lean=lean))
        assert _same(img, ref) and st["rays"] == rc["rays"], lean
        if lean:
            assert out.get(True, _counters(st)) == _counters(st)
        else:
            assert st["direct_rays"] == 0 and st["extend_rays"] == st["rays"] - st["paths"]
        out[lean] = _counters(st)
    _pin(golden, "qe-lean", out[True])


@pytest.mark.gpu
def test_megakernel_unchanged(mcpt, dr_oracle, dl_scenes):  # noqa: F811
    scene = mcpt.Scene(mcpt.ObjModel(dl_scenes["scene01"]))
    w, h, spp, chunk = FRAMES["a"]
    ref, rc = dr_oracle("scene01", "a", 2)
    img, st = scene.render(mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=chunk, max_depth=2, lean=True))
    assert _same(img, ref) and st["rays"] == rc["rays"] and st["direct_rays"] == 0 and st["extend_rays"] == 0
