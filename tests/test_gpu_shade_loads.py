"""The queue-order shade's record loads on the device (wavefront.hip wf_shade_slots,
wf_shade_item.hpp): a lane with a hit id >= 0 loads the hit's triangle record and
vertex normals in one group before the per-item code, which then takes the geometry
index, tri_hit_params' operands and scatter_n's normals from those values.  The
operations are the ones the code made before, so the check is of bits: every case
renders a frame with the megakernel (counting), with the lean wavefront and with the
counting wavefront; the three images are equal bit for bit, `rays` and `paths` are
equal, and the counting wavefront gives the megakernel's traversal counters and `shades`.

Frames of at most 64 x 64 px, 8 spp in one chunk of 8.  Each case is a place where the
loads can go wrong: every shade block size (512 beside the LDS extend on two streams,
1024 on one, 256 with the scene in global memory, where the records come from global
memory too and nothing is carried), a scene without occluder boxes (no list, no tail,
no carry), QuinEngine mode (scatter_n<true>, roulette, terminal depth 3 x max_depth),
depths 1 and 2 (terminal items dominate; a resolved terminal ray's emission), a 20 x 12
frame (kNoRay slots and lanes without an item in every group), batches that leave a
few items per segment (partial waves, empty segments, and bounce 0 through the
queue-order shade's recomputed primary rays), a camera that sees nothing (every hit id
negative: no record is loaded) and scenes of one triangle (index 0 is the only record).
"""
import numpy as np
import pytest

from test_miss_cull import _same

SPP = CHUNK = 8
COUNTERS = ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades")
AWAY = dict(eye=(0.0, 5.0, 40.0), direction=(0.0, 0.0, 1.0))          # behind the camera's back: the whole scene
ONE_MTL = "newmtl grey\nKd 0.7 0.7 0.7\nKa 0 0 0\nnewmtl glow\nKd 0.5 0.5 0.5\nKa 0.6 0.5 0.4\n"
ONE_OBJ = "mtllib one.mtl\nv -3 1 -2\nv 4 2 -1\nv 0 8 -4\nvn 0 0 1\ng tri\nusemtl %s\nf 1//1 2//1 3//1\n"
ONE_CAM = dict(eye=(0.0, 4.0, 9.0))


@pytest.fixture(scope="module")
def scenes(mcpt, tmp_path_factory):
    """(name, layout) -> the scene on the device, made once; one_grey / one_glow: a single triangle"""
    have = {}

    def get(name, layout="auto"):
        if (name, layout) not in have:
            if name.startswith("one_"):
                d = tmp_path_factory.mktemp(name)
                (d / "one.mtl").write_text(ONE_MTL)
                (d / (name + ".obj")).write_text(ONE_OBJ % name[4:])
                path = str(d / (name + ".obj"))
            else:
                path = mcpt.scene_path(name)
            have[name, layout] = mcpt.Scene(mcpt.ObjModel(path), layout=layout)
        return have[name, layout]

    yield get
    for s in have.values():
        s.close()


def _check(mcpt, scene, w=64, h=64, qe=False, sched=None, **frame):
    """megakernel == lean wavefront == counting wavefront; -> (image, megakernel counters, lean stats)"""
    make = mcpt.RenderParams.for_quinengine if qe else mcpt.RenderParams
    if qe:
        frame.setdefault("seed", 0x5EED)
    kw = dict(width=w, height=h, spp=SPP, spp_chunk=CHUNK, **frame)
    ref, rc = scene.render(make(**kw))                                  # the megakernel, counting
    lean, ls = scene.render(make(pipeline="wavefront", lean=True, **kw, **(sched or {})))
    full, fs = scene.render(make(pipeline="wavefront", lean=False, **kw, **(sched or {})))
    print({k: rc[k] for k in COUNTERS}, {k: ls[k] for k in ("direct_rays", "extend_rays", "primary_shaded")})
    assert rc["paths"] == w * h * SPP
    assert _same(lean, ref), float(np.abs(lean - ref).max())
    assert _same(full, ref), float(np.abs(full - ref).max())
    assert ls["rays"] == rc["rays"] and ls["paths"] == rc["paths"]
    for k in COUNTERS:
        assert fs[k] == rc[k], (k, fs[k], rc[k])
    return ref, rc, ls


# ---- every shade block size ---------------------------------------------------------------------

@pytest.mark.gpu
def test_default_plan_two_streams_512_thread_shade(mcpt, scenes):
    scene = scenes("scene01")
    p = mcpt.RenderParams(width=64, height=64, spp=SPP, spp_chunk=CHUNK, pipeline="wavefront", lean=True)
    assert scene.plan(p)["wf_streams"] == 2
    ref, rc, ls = _check(mcpt, scene)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    assert ls["direct_rays"] > 0                    # rays resolved where they were made: the carry's items
    assert ls["extend_rays"] + ls["direct_rays"] < rc["rays"] - rc["paths"]        # the culls dropped rays


@pytest.mark.gpu
def test_one_stream_1024_thread_shade(mcpt, scenes):
    ref, rc, ls = _check(mcpt, scenes("scene01"), sched=dict(wf_streams=1))
    assert float(ref.max()) > 0.0 and ls["direct_rays"] > 0


@pytest.mark.gpu
def test_global_layout_256_thread_shade(mcpt, scenes):
    scene = scenes("scene01", "global")
    assert scene.info()["node_boxes"] == 1
    ref, rc, ls = _check(mcpt, scene)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    assert ls["primary_shaded"] == 0                # bounce 0 through wf_shade_slots too


# ---- a scene without occluder boxes -------------------------------------------------------------

@pytest.mark.gpu
def test_closed_room_without_boxes(mcpt, scenes):
    scene = scenes("scene03")
    assert scene.info()["miss_cull_boxes"] == 0
    ref, rc, ls = _check(mcpt, scene, eye=(0.0, 5.0, 4.0))                 # inside the room
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    # no list, no tail, no carry (the room's emitter boxes still cull terminal rays, in wf_cull_terminal)
    assert ls["direct_rays"] == 0 and 0 < ls["extend_rays"] <= rc["rays"] - rc["paths"]


# ---- QuinEngine mode ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_quinengine_mode(mcpt, scenes):
    ref, rc, ls = _check(mcpt, scenes("scene01"), qe=True, max_depth=2)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    assert rc["rays"] > 3 * rc["paths"]             # paths past max_depth: the roulette's survivors


# ---- short paths --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
def test_short_paths(mcpt, scenes, depth):
    ref, rc, ls = _check(mcpt, scenes("scene01"), max_depth=depth)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    assert ls["direct_rays"] > 0                    # resolved rays, terminal ones among them at depth 1


# ---- partial tiles ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sched", [{}, dict(wf_batch=100)], ids=["default", "batch100"])
def test_partial_tiles(mcpt, scenes, sched):
    """20 x 12: three tiles by two, the right column 4 px wide and the lower row 4 px high; with
    batches of 100 paths the tiles' empty slots go through bounce 0 of the queue-order shade"""
    scene = scenes("scene01")
    w, h = 20, 12
    kw = dict(width=w, height=h, spp=SPP, spp_chunk=CHUNK)
    ref, rc = scene.render(mcpt.RenderParams(**kw))
    lean, ls = scene.render(mcpt.RenderParams(pipeline="wavefront", lean=True, **kw, **sched))
    full, fs = scene.render(mcpt.RenderParams(pipeline="wavefront", **kw, **sched))
    assert rc["paths"] == w * h * SPP and float(ref.max()) > 0.0
    assert _same(lean, ref) and _same(full, ref)
    assert ls["rays"] == rc["rays"] and ls["paths"] == rc["paths"]
    for k in COUNTERS:
        assert fs[k] == rc[k], (k, fs[k], rc[k])


# ---- short queues and partial waves -------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1000, 1280, 4096])
def test_short_queues(mcpt, scenes, batch):
    """a few items per segment at most: 1000 paths are no whole tiles (bounce 0 goes through the
    queue-order shade), 1280 are twenty; 4096 leave the later queues under a wave per segment"""
    ref, rc, ls = _check(mcpt, scenes("scene01"), sched=dict(wf_batch=batch))
    assert float(ref.max()) > 0.0
    if batch == 1000:
        assert ls["primary_shaded"] == 0


# ---- all misses ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "global"])
def test_all_misses(mcpt, scenes, layout):
    ref, rc, ls = _check(mcpt, scenes("scene01", layout), **AWAY)
    assert not ref.any() and rc["shades"] == 0 and rc["rays"] == rc["paths"]


# ---- one triangle -------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "global"])
@pytest.mark.parametrize("name", ["one_grey", "one_glow"])
def test_one_triangle(mcpt, scenes, name, layout):
    """record 0 is the only one: a grey triangle scatters (and its new rays miss), a glowing one ends
    the paths that hit it with its emission"""
    scene = scenes(name, layout)
    assert scene.info()["n_triangles"] == 1
    ref, rc, ls = _check(mcpt, scene, **ONE_CAM)
    assert rc["rays"] > 0
    if name == "one_grey":
        assert rc["shades"] > 0 and not ref.any()
    else:
        assert rc["shades"] == 0 and float(ref.max()) > 0.0
