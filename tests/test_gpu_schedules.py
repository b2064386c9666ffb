"""Scheduling never changes a result (include/mcpt.h "Scheduling"): the batch split
(`wf_batch`), the streams (`wf_streams`), the refill and ready thresholds (`wf_refill`,
`ready_thresh`), the group size of global-memory scenes (`wf_group_shift`), the
megakernel's tail split and the progressive fields (`spp_offset`, `prev_count`) --
swept here on the device, on the lean wavefront above all: primary lists, miss cull,
terminal cull, direct lists, direct resolve and clip walk, whose own tests run one
schedule each (the default: every batch the whole frame, two streams).

The oracle is the reference everywhere.  It walks every ray in full and knows nothing
of batches, streams or lists.  Every comparison is of bits and integers.

A  the wavefront, scene in LDS: scene01 (five direct-list boxes, the terminal cull,
   listed and walked tiles), the zoo's panes (direct rays, clipped rays beside full
   walks) and tetras (most walked rays clipped; tiles without a candidate),
   64 x 48 px = 48 tiles of 8 x 8, 5 spp in chunks of 2 (two full chunks and a ragged
   one), depth 3
B  the wavefront, scene in global memory: scene01 forced there, and cornell_bunny70k
C  the megakernel: scene01 in both layouts

`batch_split` restates launch_wavefront's split (wf_route.hpp) and `capacity`
make_plan's batch size (plan.cpp); each schedule's property -- why it is no duplicate of
the default -- is asserted on them without a GPU, and `capacity` against `Scene.plan`
with one.

The tile classes follow the contract of mcpt_scene_primary_tile_classes: the owned
tiles after a lean render one of whose batches was whole tiles (the candidate pass ran
and was read), (0, 0, 0) after any other render (no pass ran).  A default batch that
cuts the frame of a render that can use the lists is cut down to whole tiles; a
`wf_batch` the caller set is kept as set, which is what the schedules below rely on.
"""
import numpy as np
import pytest

from _zoo import ZOO_CAM, zoo_scenes  # noqa: F401  (zoo_scenes: a fixture)
from test_miss_cull import _same

W, H, SPP, CHUNK, DEPTH = 64, 48, 5, 2, 3
SCENES = ("scene01", "panes", "tetras")
COUNTERS = ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades")
FATE = ("direct_rays", "extend_rays", "clipped_rays")          # what became of the secondary rays


# ---- the split, restated --------------------------------------------------------------------

def owned_pixels(w, h, shard_count=1, shard_index=0, tile=8):
    """npix_local: the shard's interleaved tiles, whole (plan.cpp make_plan)"""
    ntiles = -(-w // tile) * -(-h // tile)
    owned = -(-(ntiles - shard_index) // shard_count) if shard_index < ntiles else 0
    return owned * tile * tile


def capacity(npix_local, spp, chunk, wf_batch=0, wf_streams=0, global_scene=False):
    """paths per batch and stream, before any fit to device memory (plan.cpp make_plan)"""
    chunk = min(chunk, spp) if chunk else spp
    work = max(npix_local, 1) * max(spp, chunk)
    nstr = wf_streams or (4 if global_scene else (3 if work > 1 << 29 else 2))
    big = nstr == 1 or (not global_scene and nstr == 2)
    cap = wf_batch or (1 << 28 if big else 1 << 27)
    if not wf_batch and nstr > 1:
        cap = min(cap, -(-work // nstr))
    return min(max(cap, chunk), work, 1 << 28)


def batch_split(capacity, npix_local, spp, chunk, whole=False):
    """launch_wavefront's batches in launch order: (chunk0, ncb, nsc, v0, nb) -- pixels v0 .. v0 + nb
    of the ncb chunks from chunk0 on, nsc samples each.  whole: a default batch (wf_batch 0) of a render
    that can use the primary lists (lean, CV mode, scene in LDS, tile 8) -- batches that cut the frame
    are cut down to whole tiles"""
    chunk = min(chunk, spp) if chunk else spp
    nchunks = -(-spp // chunk)
    out, c = [], 0
    while c < nchunks:
        nsc = min(spp - c * chunk, chunk)
        ncb = 1
        if nsc == chunk and npix_local * chunk <= capacity:
            ncb = min(capacity // (npix_local * chunk), spp // chunk - c)
        nb_max = capacity // (ncb * nsc)
        if whole and 64 <= nb_max < npix_local:
            nb_max -= nb_max % 64
        for v0 in range(0, npix_local, nb_max):
            out.append((c, ncb, nsc, v0, min(npix_local - v0, nb_max)))
        c += ncb
    return out


def whole_tiles(b):
    """the batch can read the primary lists: its 64-slot groups are 8 x 8 tiles"""
    return b[3] % 64 == 0 and b[4] % 64 == 0


def _split(kw, w=W, h=H, spp=SPP, chunk=CHUNK, **shard):
    npix = owned_pixels(w, h, **shard)
    cap = capacity(npix, spp, chunk, kw.get("wf_batch", 0), kw.get("wf_streams", 0))
    return cap, batch_split(cap, npix, spp, chunk)


# ---- A: schedules and the property each one has ---------------------------------------------

def _is_default(s):
    assert all(b[3] == 0 and b[4] == W * H for b in s) and len(s) == 3


def _one_stream(s):
    assert any(b[1] == 2 for b in s)                            # (and the 1024-thread shade: plan()'s wf_streams)


def _whole_with_offsets(s):
    assert all(whole_tiles(b) for b in s) and any(b[3] > 0 for b in s)
    assert {b[2]: max(x[4] for x in s if x[2] == b[2]) for b in s} == {2: 640, 1: 1280}   # ten tiles, twenty


def _mixed(s):
    """full chunks: batches of 672 px (ten and a half tiles; the last, 384 px from pixel 2688, is whole
    again); the last chunk: 1344 px = 21 tiles"""
    assert {b[2]: max(x[4] for x in s if x[2] == b[2]) for b in s} == {2: 672, 1: 1344}
    assert any(whole_tiles(b) for b in s) and any(not whole_tiles(b) for b in s)
    assert any(whole_tiles(b) and b[3] > 0 for b in s)


def _no_whole_tile(s):
    assert not any(whole_tiles(b) for b in s) and len(s) > 3


def _one_tile(s):
    full = [b for b in s if b[2] == CHUNK]
    assert len(full) == 2 * 48 and all(b[4] == 64 and b[1] * b[2] * b[4] == 128 for b in full)


def _spanning(s):
    assert any(b[1] == 2 for b in s)


SCHEDULES = {
    "default": ({}, _is_default),
    "one-stream": (dict(wf_streams=1), _one_stream),
    "streams-3": (dict(wf_streams=3, wf_batch=1280), _whole_with_offsets),
    "streams-4": (dict(wf_streams=4, wf_batch=1280), _whole_with_offsets),
    "mixed": (dict(wf_batch=1344), _mixed),
    "no-whole-tile": (dict(wf_batch=1000), _no_whole_tile),
    "one-tile": (dict(wf_batch=128), _one_tile),
    "spanning": (dict(wf_batch=1 << 22), _spanning),
}
for _r in (1, 7, 64):
    SCHEDULES["refill-%d" % _r] = (dict(wf_refill=_r), _is_default)
    SCHEDULES["refill-%d-batch-1280" % _r] = (dict(wf_refill=_r, wf_batch=1280), _whole_with_offsets)
for _n in ("one-stream", "streams-3", "mixed"):
    SCHEDULES["sorted-" + _n] = (dict(wf_sort=True, **SCHEDULES[_n][0]), SCHEDULES[_n][1])


def test_every_schedule_has_its_property():
    """without a GPU: on the restated split"""
    for name, (kw, prop) in SCHEDULES.items():
        cap, s = _split(kw)
        print(name, cap, s[:6], len(s))
        prop(s)
        assert sum(b[1] * b[2] * b[4] for b in s) == W * H * SPP, name        # every path once
    # one-pixel: an 8 x 8 frame in batches of 2 paths -- one pixel per batch in the full chunks
    cap, s = _split(dict(wf_batch=2), w=8, h=8)
    assert cap == 2 and len(s) == 64 + 64 + 32 and all(b[4] == 1 for b in s if b[2] == CHUNK)
    assert not any(whole_tiles(b) for b in s)
    # progressive: 2 spp in chunks of 1, three streams, batches of 1280 px
    cap, s = _split(dict(wf_streams=3, wf_batch=1280), spp=2, chunk=1)
    assert cap == 1280 and [b[3:] for b in s] == 2 * [(0, 1280), (1280, 1280), (2560, 512)]
    assert all(whole_tiles(b) for b in s)
    # shards: 16 tiles each, batches of 320 px in the full chunks
    for r in range(3):
        cap, s = _split(dict(wf_batch=640), shard_count=3, shard_index=r)
        assert owned_pixels(W, H, 3, r) == 1024 and cap == 640
        assert max(b[4] for b in s if b[2] == CHUNK) == 320 and all(whole_tiles(b) for b in s)
        assert any(b[3] > 0 for b in s)
    # a default batch of an odd tile count (24 x 24: nine tiles on two streams, chunks of 3, 2): cut down
    # to whole tiles where the lists can be used, work / streams as it comes where not
    npix = owned_pixels(24, 24)
    cap = capacity(npix, 5, 3)
    assert (npix, cap) == (576, 1440)
    assert [b[2:] for b in batch_split(cap, npix, 5, 3)] == [(3, 0, 480), (3, 480, 96), (2, 0, 576)]
    assert [b[2:] for b in batch_split(cap, npix, 5, 3, True)] == [(3, 0, 448), (3, 448, 128), (2, 0, 576)]
    # B: a batch smaller than two groups of 2^9
    npix = owned_pixels(W, H)
    s = batch_split(capacity(npix, SPP, CHUNK, 1000, 0, True), npix, SPP, CHUNK)
    assert all(b[1] * b[2] * b[4] < 2 << 9 for b in s)


# ---- fixtures: oracle renders and device scenes, made once ----------------------------------

def _cam(name):
    return {} if name in ("scene01", "cornell_bunny70k") else ZOO_CAM


@pytest.fixture(scope="module")
def sched_oracle(oracle_mod, mcpt, zoo_scenes):  # noqa: F811
    """-> get(scene, w, h, spp, chunk, depth, node_boxes) = the oracle's (image, counters), read-only;
    get.scene(name) = the oracle's scene"""
    have, scenes = {}, {}

    def scene(name):
        if name not in scenes:
            scenes[name] = oracle_mod.Scene(zoo_scenes[name] if name in zoo_scenes else mcpt.scene_path(name))
        return scenes[name]

    def get(name, w=W, h=H, spp=SPP, chunk=CHUNK, depth=DEPTH, node_boxes=0):
        key = (name, w, h, spp, chunk, depth, node_boxes)
        if key not in have:
            img, cnt = scene(name).render(oracle_mod.RenderParams(
                width=w, height=h, spp=spp, spp_chunk=chunk, max_depth=depth, threads=16, node_boxes=node_boxes,
                **_cam(name)))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    get.scene = scene
    return get


@pytest.fixture(scope="module")
def sched_gpu(mcpt, zoo_scenes):  # noqa: F811
    """(scene, layout) -> the scene on the device, made once"""
    have = {}

    def get(name, layout="auto"):
        if (name, layout) not in have:
            path = zoo_scenes[name] if name in zoo_scenes else mcpt.scene_path(name)
            have[name, layout] = mcpt.Scene(mcpt.ObjModel(path), layout=layout)
        return have[name, layout]

    yield get
    for s in have.values():
        s.close()


def _params(mcpt, name, lean, w=W, h=H, spp=SPP, chunk=CHUNK, depth=DEPTH, **kw):
    return mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=chunk, tile=8, max_depth=depth,
                             pipeline="wavefront", lean=lean, **_cam(name), **kw)


def _classes(scene):
    c = scene.primary_tile_classes()
    return c["empty"], c["listed"], c["walked"]


@pytest.fixture(scope="module")
def baseline(mcpt, sched_gpu):
    """scene -> the default schedule's lean stats, with the counters that say each feature fired"""
    have, classes = {}, {}

    def get(name, rc):
        if name not in have:
            scene = sched_gpu(name)
            info = scene.info()
            assert info["node_boxes"] == 0 and info["direct_list_boxes"] > 0
            _, ls = scene.render(_params(mcpt, name, True))
            cls = _classes(scene)
            secondary = rc["rays"] - rc["paths"]
            print(name, {k: ls[k] for k in FATE}, "secondary", secondary, "classes", cls)
            assert sum(cls) == W * H // 64
            assert ls["direct_rays"] > 0 or name == "tetras"
            assert 0 < ls["extend_rays"] and ls["extend_rays"] + ls["direct_rays"] < secondary     # a cull dropped rays
            if name == "scene01":
                assert info["direct_list_boxes"] == 5 and info["terminal_cull_boxes"] >= 1
                assert cls[1] > 0 and cls[2] > 0, cls     # listed and walked tiles (this frame: none is empty)
            elif name == "panes":
                assert 0 < ls["clipped_rays"] < ls["extend_rays"]
            else:
                assert ls["clipped_rays"] > 0.5 * ls["extend_rays"]
            have[name] = ls
            classes[name] = cls
        return have[name]

    get.classes = classes
    return get


def _check_wavefront(mcpt, scene, name, kw, ref, rc, base=None, global_scene=False, frame=None):
    """a lean and a counting render under schedule kw against the oracle's (ref, rc); -> the split"""
    frame = frame or {}
    fw, fh = frame.get("w", W), frame.get("h", H)
    fspp, fchunk = frame.get("spp", SPP), frame.get("chunk", CHUNK)
    npix = owned_pixels(fw, fh)
    cap = capacity(npix, fspp, fchunk, kw.get("wf_batch", 0), kw.get("wf_streams", 0), global_scene)
    split = batch_split(cap, npix, fspp, fchunk, whole=not global_scene and "wf_batch" not in kw)   # (the lean render's)
    listed = not global_scene and any(whole_tiles(b) for b in split)
    for lean in (True, False):
        p = _params(mcpt, name, lean, **frame, **kw)
        pl = scene.plan(p)
        assert pl["wf_batch"] == cap, (pl["wf_batch"], cap)
        assert pl["wf_queue_bytes"] < 8 << 30
        for k in ("wf_streams", "wf_refill", "wf_group_shift"):
            assert not kw.get(k) or pl[k] == kw[k], (k, pl[k])
        img, st = scene.render(p)
        cls = _classes(scene)
        print("lean" if lean else "counting", {k: st[k] for k in COUNTERS + FATE}, "classes", cls)
        assert _same(img, ref), (lean, float(np.abs(img - ref).max()))
        for k in ("rays", "paths", "shades"):
            assert st[k] == rc[k], (lean, k, st[k], rc[k])
        if lean:
            assert (sum(cls) == npix // 64) if listed else (cls == (0, 0, 0)), (cls, listed)
            if base is not None:
                assert {k: st[k] for k in FATE} == {k: base[k] for k in FATE}
        else:
            assert cls == (0, 0, 0)
            for k in COUNTERS:
                assert st[k] == rc[k], (k, st[k], rc[k])
            assert st["direct_rays"] == 0 == st["clipped_rays"]
            assert st["extend_rays"] == rc["rays"] - rc["paths"]
    return split


# ---- A: the wavefront, scene in LDS ---------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", SCENES)
def test_lds_wavefront_schedule(mcpt, sched_oracle, sched_gpu, baseline, name, sched):
    kw, prop = SCHEDULES[sched]
    ref, rc = sched_oracle(name)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    base = baseline(name, rc)
    prop(_check_wavefront(mcpt, sched_gpu(name), name, kw, ref, rc, base))


@pytest.mark.gpu
def test_the_scenes_hold_all_three_tile_classes(sched_oracle, baseline):
    """scene01's box fills the 64 x 48 frame (listed and walked tiles only); the zoo's frames add
    the tiles without a candidate, which make no primary ray"""
    for name in SCENES:
        baseline(name, sched_oracle(name)[1])
    assert all(max(baseline.classes[n][k] for n in SCENES) > 0 for k in range(3)), baseline.classes


@pytest.mark.gpu
def test_one_pixel_batches(mcpt, sched_oracle, sched_gpu):
    """one tile, 2 paths per batch: 64 batches of one pixel per full chunk, 32 of two in the last"""
    ref, rc = sched_oracle("scene01", w=8, h=8)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0 and rc["rays"] > rc["paths"]
    s = _check_wavefront(mcpt, sched_gpu("scene01"), "scene01", dict(wf_batch=2), ref, rc, frame=dict(w=8, h=8))
    assert len(s) == 160 and not any(whole_tiles(b) for b in s)


@pytest.mark.gpu
def test_default_batches_of_an_odd_tile_count_are_whole_tiles(mcpt, sched_oracle, sched_gpu):
    """24 x 24 px, 5 spp in chunks of 3: work / streams is seven and a half tiles of 3 samples; the lean
    render's batches hold seven tiles and two, and read the lists"""
    frame = dict(w=24, h=24, spp=5, chunk=3)
    ref, rc = sched_oracle("scene01", **frame)
    assert float(ref.max()) > 0.0 and rc["rays"] > rc["paths"]
    s = _check_wavefront(mcpt, sched_gpu("scene01"), "scene01", {}, ref, rc, frame=frame)
    assert all(whole_tiles(b) for b in s) and any(b[3] > 0 for b in s)


@pytest.mark.gpu
def test_progressive_calls_on_three_streams(mcpt, oracle_mod, sched_oracle, sched_gpu):
    """three calls of 2 spp continuing one running mean, each in batches of 1280 px on three streams"""
    scene, osc = sched_gpu("scene01"), sched_oracle.scene("scene01")
    img = np.zeros((H, W, 3), np.float32)
    ref = np.zeros((H, W, 3), np.float32)
    for k in range(3):
        p = _params(mcpt, "scene01", True, spp=2, chunk=1, spp_offset=2 * k, prev_count=k, wf_streams=3, wf_batch=1280)
        pl = scene.plan(p)
        assert (pl["wf_streams"], pl["wf_batch"]) == (3, 1280)
        _, st = scene.render(p, img)
        ref, rc = osc.render(oracle_mod.RenderParams(width=W, height=H, spp=2, spp_chunk=1, max_depth=DEPTH, threads=16,
                                                     spp_offset=2 * k, prev_count=k), ref)
        assert _same(img, ref), k
        assert st["rays"] == rc["rays"] and st["paths"] == rc["paths"] and st["shades"] == rc["shades"]
        assert sum(_classes(scene)) == 48
    assert float(ref.max()) > 0.0


@pytest.mark.gpu
def test_three_packed_shards_in_small_batches(mcpt, sched_oracle, sched_gpu, baseline):
    ref, rc = sched_oracle("scene01")
    base = baseline("scene01", rc)
    scene = sched_gpu("scene01")
    got = np.full((H, W, 3), -1.0, np.float32)
    tot = dict.fromkeys(("rays", "paths", "shades") + FATE, 0)
    for r in range(3):
        p = _params(mcpt, "scene01", True, shard_count=3, shard_index=r, packed=True, wf_batch=640)
        assert scene.plan(p)["wf_batch"] == 640
        part, st = scene.render(p)
        assert sum(_classes(scene)) == 16
        for k in tot:
            tot[k] += st[k]
        xy = p.shard_pixels()
        assert len(xy) == 1024
        ok = xy[:, 0] >= 0
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
    assert _same(got, ref)
    assert {k: tot[k] for k in ("rays", "paths", "shades")} == {k: rc[k] for k in ("rays", "paths", "shades")}
    assert {k: tot[k] for k in FATE} == {k: base[k] for k in FATE}


# ---- B: the wavefront, scene in global memory -----------------------------------------------

GLOBAL_FRAMES = {"scene01": dict(), "cornell_bunny70k": dict(w=40, h=32, spp=3, chunk=2)}
GLOBAL_SCHEDULES = {
    "shift-6-one-stream": dict(wf_group_shift=6, wf_streams=1),
    "shift-9-one-stream": dict(wf_group_shift=9, wf_streams=1),
    "shift-14-one-stream": dict(wf_group_shift=14, wf_streams=1),       # (at most 2 streams: the queues' size)
    "shift-6-streams-4": dict(wf_group_shift=6, wf_streams=4),
    "shift-9-streams-4": dict(wf_group_shift=9, wf_streams=4),
    "refill-1": dict(wf_refill=1),
    "refill-64": dict(wf_refill=64),
    "batch-1000-shift-9": dict(wf_batch=1000, wf_group_shift=9),        # less than two groups
}


@pytest.mark.gpu
@pytest.mark.parametrize("sched", sorted(GLOBAL_SCHEDULES))
@pytest.mark.parametrize("name", sorted(GLOBAL_FRAMES))
def test_global_wavefront_schedule(mcpt, sched_oracle, sched_gpu, name, sched):
    scene = sched_gpu(name, "global")
    assert scene.info()["node_boxes"] == 1
    frame = GLOBAL_FRAMES[name]
    ref, rc = sched_oracle(name, node_boxes=1, **frame)
    assert float(ref.max()) > 0.0 and rc["rays"] > rc["paths"]
    kw = GLOBAL_SCHEDULES[sched]
    s = _check_wavefront(mcpt, scene, name, kw, ref, rc, global_scene=True, frame=frame)
    if "wf_batch" in kw:
        assert all(b[1] * b[2] * b[4] < 2 << kw["wf_group_shift"] for b in s)


# ---- C: the megakernel ----------------------------------------------------------------------

MK = dict(width=40, height=30, spp=4, spp_chunk=2)
MK_UNITS = owned_pixels(40, 30) * 2                                      # 1280 px (20 tiles) x 2 chunks
MK_TAILS = {"tail-default": {}, "tail-off": dict(tail_units_per_lane=-1), "tail-mixed": dict(tail_units=1000)}


def test_mixed_tail_leaves_both_kinds_of_unit():
    assert 0 < MK_TAILS["tail-mixed"]["tail_units"] < MK_UNITS == 2560


@pytest.mark.gpu
@pytest.mark.parametrize("tail", sorted(MK_TAILS))
@pytest.mark.parametrize("ready", [1, 33, 64])
@pytest.mark.parametrize("layout", ["auto", "global"])
def test_megakernel_schedule(mcpt, sched_oracle, sched_gpu, layout, ready, tail):
    scene = sched_gpu("scene01", layout)
    boxes = int(layout == "global")
    assert scene.info()["node_boxes"] == boxes
    ref, rc = sched_oracle("scene01", w=40, h=30, spp=4, chunk=2, depth=7, node_boxes=boxes)
    assert float(ref.max()) > 0.0
    kw = dict(ready_thresh=ready, **MK_TAILS[tail])
    pl = scene.plan(mcpt.RenderParams(**MK, **kw))
    assert pl["pipeline"] == 0 and pl["ready_thresh"] == ready
    if tail != "tail-default":
        assert pl["tail_units"] == kw.get("tail_units", 0)
    img, st = scene.render(mcpt.RenderParams(**MK, **kw))
    assert _same(img, ref), float(np.abs(img - ref).max())
    for k in COUNTERS:
        assert st[k] == rc[k], (k, st[k], rc[k])
    lean, ls = scene.render(mcpt.RenderParams(lean=True, **MK, **kw))
    assert _same(lean, ref) and ls["rays"] == rc["rays"]
