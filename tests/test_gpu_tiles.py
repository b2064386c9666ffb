"""Tile sizes other than 8 on the GPU (mcpt_render_params::tile, 1..256), and a
shard that owns no tile.

The image does not depend on the tile: the RNG is keyed by (pixel, sample) and
the sums are per pixel in chunk order.  So every case is compared with the CPU
oracle's ordered walk (as tests/test_gpu_parity.py), bit for bit and counter for
counter.  The frames make the packed pixel count (owned tiles x tile^2) awkward:
no multiple of 64 for the small tiles, mostly padding for the large ones, so the
unit_pixel decode runs with divisors other than 64 / 8, and the reduction, the
gather and the wavefront's 64-path groups run with partly filled waves.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades")
# tile: (W, H, packed pixels)
FRAMES = {1: (37, 29, 1073), 3: (37, 29, 1170), 4: (36, 28, 1008), 5: (37, 29, 1200), 16: (37, 29, 1536),
          32: (37, 29, 2048), 256: (20, 12, 65536)}
SPP, CHUNK = 5, 2

_scenes = {}
_oracle = {}


def _flavor(name):
    return "tinyobj" if name.startswith("qe_") else "cvmctracer"


def _scene(mcpt, name="scene01"):
    if name not in _scenes:
        _scenes[name] = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name), flavor=_flavor(name)))
    return _scenes[name]


def _scene_id(name):
    return 2 if name in ("scene02", "scene03") else 1


def _ref(mcpt, oracle_mod, name, W, H, spp=SPP, chunk=CHUNK, offset=0, prev=None, prev_count=0, qe=None):
    """the oracle's ordered walk (image, counters); first renders are computed once and left unchanged"""
    key = (name, W, H, spp, chunk, offset, qe)
    if prev is None and key in _oracle:
        return _oracle[key]
    path = mcpt.scene_path(name)
    boxes = int(mcpt.Scene(mcpt.ObjModel(path, flavor=_flavor(name)), host_only=True).info()["node_boxes"])
    o = oracle_mod.Scene(path, flavor=_flavor(name))
    if qe is not None:
        depth, seed = qe
        p = oracle_mod.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, max_depth=depth, seed=seed, illum=1.0,
                                    fov=45.0, fresnel_kd=0, threads=8, mode=oracle_mod.MODE_QE, node_boxes=boxes)
    else:
        p = oracle_mod.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, scene_id=_scene_id(name),
                                    traversal=oracle_mod.KD_ORDERED, threads=8, spp_offset=offset,
                                    prev_count=prev_count, node_boxes=boxes)
    img, rc = o.render(p, None if prev is None else prev.copy())
    if prev is None:
        img.setflags(write=False)
        _oracle[key] = (img, rc)
    return img, rc


def _packed(mcpt, T):
    """the packed pixel list of tile T's frame, with the coverage the cases rely on asserted"""
    W, H, n = FRAMES[T]
    xy = mcpt.RenderParams(width=W, height=H, tile=T, packed=True).shard_pixels()
    assert len(xy) == n
    if T in (1, 3, 4, 5):
        assert n % 64 != 0 and n % 256 != 0            # a partly filled last wave and workgroup
    if T in (16, 32, 256):
        assert (xy[:, 0] < 0).any()                    # padding
        assert n % (T * T) == 0 and n // (T * T) == ((W + T - 1) // T) * ((H + T - 1) // T)
    assert int((xy[:, 0] >= 0).sum()) == W * H
    return xy


def _params(mcpt, name, T, pipeline="megakernel", **kw):
    W, H, _ = FRAMES[T]
    base = dict(width=W, height=H, spp=SPP, spp_chunk=CHUNK, tile=T,
                pipeline="wavefront" if pipeline.startswith("wavefront") else pipeline,
                wf_sort=pipeline == "wavefront-sorted")
    base.update(kw)
    return mcpt.RenderParams.for_scene(_scene_id(name), **base)


def _assert_image(img, ref):
    bad = (img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), img[bad][:5].tolist(), ref[bad][:5].tolist())


def _assert_counters(st, rc, names=COUNTERS):
    assert {k: st[k] for k in names} == {k: rc[k] for k in names}


PIPELINE_CASES = [(T, pl) for T in FRAMES for pl in ("megakernel", "wavefront", "wavefront-sorted")
                  if not (T == 256 and pl == "wavefront-sorted")]


@pytest.mark.parametrize("T,pipeline", PIPELINE_CASES, ids=[f"tile{T}-{pl}" for T, pl in PIPELINE_CASES])
def test_every_tile_renders_the_oracle_image(mcpt, oracle_mod, T, pipeline):
    _packed(mcpt, T)
    W, H, _ = FRAMES[T]
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    img, st = _scene(mcpt).render(_params(mcpt, "scene01", T, pipeline))
    assert st["variant"] in ((1, 2, 3) if pipeline == "megakernel" else (4, 5))
    _assert_image(img, ref)
    _assert_counters(st, rc)


@pytest.mark.parametrize("tk", [dict(tail_units_per_lane=-1), dict(tail_units=1000)], ids=["whole-units", "mixed"])
def test_tail_split_with_tile_5(mcpt, oracle_mod, tk):
    """1200 packed pixels x 3 chunks = 3600 units: none, or the last 1000, handed out by sample"""
    _packed(mcpt, 5)
    W, H, _ = FRAMES[5]
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    img, st = _scene(mcpt).render(_params(mcpt, "scene01", 5, **tk))
    _assert_image(img, ref)
    _assert_counters(st, rc)


@pytest.mark.parametrize("T", [4, 5])
def test_wavefront_batches_of_1000_paths(mcpt, oracle_mod, T):
    """wf_batch 1000 at chunks of 2: batches of 500 pixels, no multiple of 64, so a 64-path group
    straddles two samples and a sample's last group is partial; the packed count is no multiple
    of 500 either"""
    n = len(_packed(mcpt, T))
    assert (1000 // CHUNK) % 64 != 0 and n % (1000 // CHUNK) != 0
    W, H, _ = FRAMES[T]
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    for sort in (False, True):
        img, st = _scene(mcpt).render(_params(mcpt, "scene01", T, "wavefront", wf_batch=1000, wf_sort=sort))
        _assert_image(img, ref)
        _assert_counters(st, rc)


@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
@pytest.mark.parametrize("T", [4, 5])
def test_global_memory_scene(mcpt, oracle_mod, T, pipeline):
    """scene03 is served from global memory: the other megakernel variant, and the wavefront's
    generate kernel and XCD dealing"""
    _packed(mcpt, T)
    W, H, _ = FRAMES[T]
    scene = _scene(mcpt, "scene03")
    assert int(scene.info()["node_boxes"]) == 1
    ref, rc = _ref(mcpt, oracle_mod, "scene03", W, H)
    img, st = scene.render(_params(mcpt, "scene03", T, pipeline))
    assert st["variant"] == (3 if pipeline == "megakernel" else 5)
    _assert_image(img, ref)
    _assert_counters(st, rc)


@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_quinengine_mode_with_tile_4(mcpt, oracle_mod, pipeline):
    _packed(mcpt, 4)
    W, H, _ = FRAMES[4]
    ref, rc = _ref(mcpt, oracle_mod, "qe_scene01", W, H, spp=3, chunk=2, qe=(5, 1234))
    p = mcpt.RenderParams.for_quinengine(width=W, height=H, spp=3, spp_chunk=2, max_depth=5, seed=1234, tile=4,
                                         pipeline=pipeline)
    img, st = _scene(mcpt, "qe_scene01").render(p)
    _assert_image(img, ref)
    _assert_counters(st, rc)


def test_progressive_prev_count_chain_with_tile_4(mcpt, oracle_mod):
    _packed(mcpt, 4)
    W, H, _ = FRAMES[4]
    img = np.zeros((H, W, 3), np.float32)
    ref = np.zeros((H, W, 3), np.float32)
    for k in range(3):
        _scene(mcpt).render(mcpt.RenderParams(width=W, height=H, spp=3, spp_chunk=2, spp_offset=3 * k, prev_count=k,
                                              tile=4), img)
        ref, _ = _ref(mcpt, oracle_mod, "scene01", W, H, spp=3, chunk=2, offset=3 * k, prev=ref, prev_count=k)
        _assert_image(img, ref)


def _unit_order(mcpt, W, H, tile):
    """row-major pixel index -> work-unit pixel index v (tile-major, render.hip unit_pixel)"""
    xy = mcpt.RenderParams(width=W, height=H, tile=tile, packed=True).shard_pixels()
    inv = np.full(W * H, -1, np.int64)
    ok = xy[:, 0] >= 0
    inv[xy[ok, 1] * W + xy[ok, 0]] = np.nonzero(ok)[0]
    assert (inv >= 0).all()
    return inv, len(xy), ok


def _pixel_counters(mcpt, W, H, tile):
    """(H * W, 4) uint64 rays, inner, leaf, tests per pixel (summed over the chunks), and the packed image"""
    inv, npk, ok = _unit_order(mcpt, W, H, tile)
    nch = (SPP + CHUNK - 1) // CHUNK
    fb, uc = _scene(mcpt).render_unit_counters(mcpt.RenderParams(width=W, height=H, spp=SPP, spp_chunk=CHUNK,
                                                                 tile=tile, packed=True))   # one slot per unit pixel
    assert uc.shape == (npk * nch, 4) and fb.shape == (npk, 3)
    per = uc.reshape(nch, npk, 4).astype(np.uint64).sum(axis=0)
    assert (per[~ok] == 0).all()                       # padding does no work
    return per[inv], fb[inv]


@pytest.mark.parametrize("T", [4, 16])
def test_per_unit_counters_are_those_of_tile_8_pixel_by_pixel(mcpt, oracle_mod, T):
    _packed(mcpt, T)
    W, H, _ = FRAMES[T]
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    got, fb = _pixel_counters(mcpt, W, H, T)
    want, fb8 = _pixel_counters(mcpt, W, H, 8)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=1))[:5].tolist()
    _assert_image(fb.reshape(H, W, 3), ref)
    _assert_image(fb8.reshape(H, W, 3), ref)
    tot = got.sum(axis=0)
    for i, k in enumerate(("rays", "inner_visits", "leaf_visits", "tri_tests")):
        assert int(tot[i]) == rc[k], (k, int(tot[i]), rc[k])


def test_unit_counters_refuse_the_wavefront_and_leave_the_scene_usable(mcpt, oracle_mod):
    """Per-unit counters exist on the megakernel only: the wavefront refuses them
    with MCPT_E_UNSUPPORTED before anything is launched, and the scene's next
    render is the oracle's image with the oracle's counters."""
    from montecarlopathtracer_amd._capi import McptError
    W, H, _ = FRAMES[4]
    with pytest.raises(McptError, match="unit counters need the megakernel pipeline") as e:
        _scene(mcpt).render_unit_counters(_params(mcpt, "scene01", 4, "wavefront"))
    assert e.value.code == -6
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    img, st = _scene(mcpt).render(_params(mcpt, "scene01", 4, "wavefront"))
    _assert_image(img, ref)
    _assert_counters(st, rc)


@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
@pytest.mark.parametrize("T", [4, 5])
def test_three_shards_reassemble_the_image(mcpt, oracle_mod, T, pipeline):
    _packed(mcpt, T)
    W, H, _ = FRAMES[T]
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    full, _ = _scene(mcpt).render(_params(mcpt, "scene01", T, pipeline))
    got = np.full((H, W, 3), -1.0, np.float32)
    tot = dict.fromkeys(COUNTERS, 0)
    for r in range(3):
        p = _params(mcpt, "scene01", T, pipeline, shard_count=3, shard_index=r)
        part, st = _scene(mcpt).render(p)
        xy = p.shard_pixels()
        assert part.shape == (len(xy), 3)
        ok = xy[:, 0] >= 0
        assert (part[~ok] == 0).all()                  # padding slots are not written
        got[xy[ok, 1], xy[ok, 0]] = part[ok]
        for k in COUNTERS:
            tot[k] += st[k]
    _assert_image(got, full)
    _assert_image(got, ref)
    _assert_counters(tot, rc)


@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_packed_output_with_tile_5_is_the_permuted_image(mcpt, oracle_mod, pipeline):
    xy = _packed(mcpt, 5)
    W, H, _ = FRAMES[5]
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    full, _ = _scene(mcpt).render(_params(mcpt, "scene01", 5, pipeline))
    packed, st = _scene(mcpt).render(_params(mcpt, "scene01", 5, pipeline, packed=True))
    ok = xy[:, 0] >= 0
    assert packed.shape == (len(xy), 3) and (packed[~ok] == 0).all()
    _assert_image(packed[ok], full[xy[ok, 1], xy[ok, 0]])
    _assert_image(full, ref)
    _assert_counters(st, rc)


# ---- multi-device lists ---------------------------------------------------------------

@pytest.fixture
def devices(mcpt):
    """set a device list for this test's scenes, restore [0] afterwards"""
    tr = mcpt.Tracer()
    yield tr.initialize
    tr.initialize([0])


@pytest.mark.parametrize("force_peer_copy", [False, True], ids=["gather", "peer-copy"])
@pytest.mark.parametrize("T", [4, 32])
@pytest.mark.parametrize("n", [2, 3])
def test_replicas_render_the_single_device_image(mcpt, oracle_mod, devices, n, T, force_peer_copy):
    W, H = 37, 29
    empty = [r for r in range(n)
             if mcpt.RenderParams(width=W, height=H, tile=T, shard_count=n, shard_index=r).output_pixels() == 0]
    if T == 32 and n == 3:
        assert empty == [2]                            # two tiles, three devices: shard 2 owns none
    else:
        assert not empty
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    devices([0] * n)
    multi = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    assert multi.info()["n_devices"] == n
    for pipeline in ("megakernel", "wavefront"):
        kw = dict(width=W, height=H, spp=SPP, spp_chunk=CHUNK, tile=T, pipeline=pipeline,
                  force_peer_copy=force_peer_copy)
        img0, st = multi.render(mcpt.RenderParams(**kw))
        assert st["devices"] == n
        _assert_image(img0, ref)
        _assert_counters(st, rc)
        # progressive second call: the gather applies the running mean
        ref1, _ = _ref(mcpt, oracle_mod, "scene01", W, H, offset=SPP, prev=ref, prev_count=1)
        img1, _ = multi.render(mcpt.RenderParams(spp_offset=SPP, prev_count=1, **kw), img0.copy())
        _assert_image(img1, ref1)


@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_rccl_gather_one_device_with_tile_5(mcpt, oracle_mod, devices, pipeline):
    _packed(mcpt, 5)
    W, H, _ = FRAMES[5]
    ref, rc = _ref(mcpt, oracle_mod, "scene01", W, H)
    devices([0])
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    img, st = scene.render(_params(mcpt, "scene01", 5, pipeline, gather="rccl"))
    _assert_image(img, ref)
    _assert_counters(st, rc)


# ---- a shard that owns no tile ----------------------------------------------------------

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_a_shard_without_tiles_renders_nothing(mcpt, pipeline):
    """20x12 at tile 8 has six tiles; shard 7 of 8 owns none: the call succeeds, nothing is
    written, no ray is traced -- on the host entry and on the device entry"""
    import torch
    W, H = 20, 12
    kw = dict(width=W, height=H, spp=SPP, spp_chunk=CHUNK, tile=8, shard_count=8, pipeline=pipeline)
    counts = [mcpt.RenderParams(shard_index=r, **kw).output_pixels() for r in range(8)]
    assert counts == [64] * 6 + [0, 0]
    p = mcpt.RenderParams(shard_index=7, **kw)
    assert p.shard_pixels().shape == (0, 2)
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    img, st = scene.render(p)
    assert img.shape == (0, 3)
    assert st["renders"] == 1 and st["rays"] == 0 and st["paths"] == 0 and st["shades"] == 0
    fb = torch.full((64, 4), -1.0, device="cuda")
    torch.cuda.synchronize()
    scene.render_device(p, fb.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = scene.stats()
    assert bool((fb == -1.0).all())
    assert st["renders"] == 1 and st["rays"] == 0 and st["paths"] == 0
    # the scene still renders: an owning shard afterwards, against the unsharded image
    full, _ = scene.render(mcpt.RenderParams(width=W, height=H, spp=SPP, spp_chunk=CHUNK, pipeline=pipeline))
    p5 = mcpt.RenderParams(shard_index=5, **kw)
    part, st5 = scene.render(p5)
    xy = p5.shard_pixels()
    ok = xy[:, 0] >= 0
    _assert_image(part[ok], full[xy[ok, 1], xy[ok, 0]])
    assert st5["paths"] == SPP * int(ok.sum())
