"""GPU path at BASELINE sizes, through size-independent properties, plus the
statistical pin against the reference's own 1000-spp render.

* 512x512 @ 16 spp (BASELINE configs[0], C1) as a whole frame: bit-identical
  to the CPU oracle, counters equal.
* 1024x1024 @ 1024 spp (BASELINE configs[1]): rendering the 8 interleaved
  tile shards (configs[2]'s partition) and reassembling them reproduces the
  single-GPU image bit for bit; a second render is bit-identical (determinism);
  the image is finite and the light is the brightest region.
* the same frame through the wavefront pipeline: bit-identical image, equal
  counters; and C5 (4096 spp) likewise, twice (determinism); the C2 frame's
  2 and 8 packed shards and C5's 8 (one rank's work in bench.py's N-GPU runs)
  reassemble them.
* every BASELINE config at its own sample count against the oracle: 128x128
  crops of the whole C2 frame (light, glass sphere, miss corner), a 32x32 crop
  of C4 (1024 spp), a 64x64 crop of C5 (4096 spp), both pipelines, bit for bit, with the
  megakernel's per-unit counters summed over the crop equal to the oracle's.
* RenderScene's progressive loop (10 launches x 100 spp, prevCount running
  mean, CUTracer.cu:378-398) at 800x600 with the published-render variant
  (luminance 30, untinted Fresnel) matches CV/result1.png statistically.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def scene01(mcpt):
    return mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))


def test_fullsize_shards_and_determinism(mcpt, scene01):
    import torch
    W = H = 1024
    p = mcpt.RenderParams(width=W, height=H, spp=1024, spp_chunk=32)
    full = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    scene01.render_device(p, full.data_ptr(), torch.cuda.current_stream().cuda_stream)
    again = torch.zeros_like(full)
    scene01.render_device(p, again.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = scene01.stats()
    assert st["renders"] == 2 and st["rays"] > 2 * 3.0e9
    assert torch.equal(full, again)
    img = full.view(H, W, 4)[..., :3].cpu().numpy()
    assert np.isfinite(img).all() and img.min() >= 0
    b = img.mean(axis=2).reshape(32, 32, 32, 32).mean(axis=(1, 3))     # 32x32-pixel blocks
    by, bx = np.unravel_index(np.argmax(b), b.shape)
    assert b.max() > 5 * img.mean() and by < 12 and 10 <= bx <= 21      # ceiling light, centred, upper part
    N = 8
    got = torch.full((H * W, 4), -1.0, dtype=torch.float32, device="cuda")
    for r in range(N):
        ps = mcpt.RenderParams(width=W, height=H, spp=1024, spp_chunk=32, shard_count=N, shard_index=r)
        part = torch.zeros((ps.output_pixels(), 4), dtype=torch.float32, device="cuda")
        scene01.render_device(ps, part.data_ptr(), torch.cuda.current_stream().cuda_stream)
        xy = torch.from_numpy(ps.shard_pixels().astype(np.int64)).cuda()
        ok = xy[:, 0] >= 0
        got[(xy[:, 1] * W + xy[:, 0])[ok]] = part[ok]
    torch.cuda.synchronize()
    scene01.stats()
    assert torch.equal(got[:, :3], full[:, :3])


@pytest.mark.parametrize("N", [2, 8])
def test_fullsize_wavefront_shards_reassemble(mcpt, scene01, N):
    """What one rank of bench.py's N-GPU run renders (the wavefront, packed
    interleaved tiles, default batches = work / streams, implicit queue 0 with
    the shard's pixel mapping): the N shards reassemble the whole-frame image
    bit for bit."""
    import torch
    W = H = 1024
    p = mcpt.RenderParams(width=W, height=H, spp=1024, spp_chunk=32, pipeline="wavefront")
    full = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    scene01.render_device(p, full.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = torch.full((H * W, 4), -1.0, dtype=torch.float32, device="cuda")
    for r in range(N):
        ps = mcpt.RenderParams(width=W, height=H, spp=1024, spp_chunk=32, shard_count=N, shard_index=r,
                               packed=True, tile=8, pipeline="wavefront")
        part = torch.zeros((ps.output_pixels(), 4), dtype=torch.float32, device="cuda")
        scene01.render_device(ps, part.data_ptr(), torch.cuda.current_stream().cuda_stream)
        xy = torch.from_numpy(ps.shard_pixels().astype(np.int64)).cuda()
        ok = xy[:, 0] >= 0
        got[(xy[:, 1] * W + xy[:, 0])[ok]] = part[ok]
    torch.cuda.synchronize()
    scene01.stats()
    assert torch.equal(got[:, :3], full[:, :3])


def test_c1_full_frame_bit_identical_to_oracle(mcpt, oracle_mod, scene01):
    """BASELINE configs[0] (C1: 512x512, 16 spp, the reference's CPU-runnable
    case) as one whole frame: the device image equals the CPU oracle's ordered
    walk bit for bit, with equal ray / path / visit / test / shade counts
    (~14 M closest-hit queries)."""
    W = H = 512
    p = mcpt.RenderParams(width=W, height=H, spp=16)
    img, st = scene01.render(p)
    o = oracle_mod.Scene(mcpt.scene_path("scene01"))
    ref, rc = o.render(oracle_mod.RenderParams(width=W, height=H, spp=16, spp_chunk=p.spp_chunk,
                                               traversal=oracle_mod.KD_ORDERED, threads=16))
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), float(np.abs(img - ref).max())
    for k in ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades"):
        assert st[k] == rc[k], (k, st[k], rc[k])
    assert st["rays"] > 1.3e7


def _host_threads() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def _unit_order(mcpt, W, H, tile=8):
    """row-major pixel index -> work-unit pixel index v (tile-major, render.hip unit_pixel)"""
    xy = mcpt.RenderParams(width=W, height=H, tile=tile, packed=True).shard_pixels()
    inv = np.full(W * H, -1, np.int64)
    ok = xy[:, 0] >= 0
    inv[xy[ok, 1] * W + xy[ok, 0]] = np.nonzero(ok)[0]
    return inv


def _crop_counters(uc, inv, npix, region, W):
    """sum of the per-unit counters {rays, inner, leaf, tests} over a crop's pixels, all chunks"""
    x0, y0, x1, y1 = region
    pix = (np.arange(y0, y1)[:, None] * W + np.arange(x0, x1)[None, :]).ravel()
    v = inv[pix]
    nch = uc.shape[0] // npix
    units = (np.arange(nch)[:, None] * npix + v[None, :]).ravel()
    return uc[units].astype(np.uint64).sum(axis=0)


@pytest.fixture(scope="module")
def c2_frames(mcpt, scene01):
    """BASELINE configs[1] (C2: 1024x1024, 1024 spp in 32-sample chunks) rendered
    whole by the megakernel with per-unit counters and by the (default)
    wavefront pipeline"""
    W = H = 1024
    p = mcpt.RenderParams(width=W, height=H, spp=1024, spp_chunk=32)
    mk, uc = scene01.render_unit_counters(p)
    _, smk = scene01.render(p)                      # whole-frame counters (tail split on)
    wf, swf = scene01.render(mcpt.RenderParams(width=W, height=H, spp=1024, spp_chunk=32, pipeline="wavefront"))
    return {"mega": mk.reshape(H, W, 3), "uc": uc, "wave": wf, "st_mega": smk, "st_wave": swf}


def test_fullsize_pipelines_agree(c2_frames):
    """C2 at full size through two independent implementations: the wavefront
    pipeline (per-bounce queues) renders the megakernel's image bit for bit,
    with equal work counters."""
    assert np.array_equal(c2_frames["wave"], c2_frames["mega"])
    for k in ("rays", "paths", "inner_visits", "leaf_visits", "tri_tests", "shades"):
        assert c2_frames["st_wave"][k] == c2_frames["st_mega"][k], k
    assert c2_frames["uc"][:, 0].astype(np.uint64).sum() == c2_frames["st_mega"]["rays"]


# crops of the C2 frame: the ceiling light, the glass sphere on the floor, and
# the upper-left corner (misses above the box beside the red wall)
C2_CROPS = {"light": (448, 192, 576, 320), "glass_sphere": (576, 640, 704, 768), "miss_corner": (0, 64, 128, 192)}


@pytest.mark.parametrize("crop", sorted(C2_CROPS))
def test_c2_full_spp_crops_match_oracle(mcpt, oracle_mod, c2_frames, crop):
    """The headline frame at its own sample count (1024 spp, 32 chunks reduced in
    chunk order, CUTracer.cu:192-217 with the launch loop's sums): 128x128 crops
    of both pipelines' whole-frame renders equal the oracle's region render bit
    for bit, and the megakernel's per-unit counters summed over the crop equal
    the oracle's rays / inner / leaf visits / triangle tests there."""
    W = 1024
    x0, y0, x1, y1 = C2_CROPS[crop]
    o = oracle_mod.Scene(mcpt.scene_path("scene01"))
    ref, rc = o.render(oracle_mod.RenderParams(width=W, height=W, spp=1024, spp_chunk=32,
                                               traversal=oracle_mod.KD_ORDERED, threads=_host_threads(),
                                               region=(x0, y0, x1, y1)))
    want = ref[y0:y1, x0:x1]
    for name in ("mega", "wave"):
        got = c2_frames[name][y0:y1, x0:x1]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, float(np.abs(got - want).max()))
    cc = _crop_counters(c2_frames["uc"], _unit_order(mcpt, W, W), W * W, (x0, y0, x1, y1), W)
    assert [int(x) for x in cc] == [rc["rays"], rc["inner_visits"], rc["leaf_visits"], rc["tri_tests"]]
    assert rc["rays"] > 128 * 128 * 1024 * (1.05 if crop == "miss_corner" else 2.0)


def test_c4_full_spp_crop_matches_oracle(mcpt, oracle_mod):
    """BASELINE configs[3] (the 70k-triangle mesh, scene image in global memory,
    child-box cull) at 1024 spp: a 32x32 crop over the mesh's silhouette of both
    pipelines' whole frames equals the oracle's node-box walk bit for bit;
    megakernel unit counters over the crop equal the oracle's."""
    W = 1024
    path = mcpt.scene_path("cornell_bunny70k")
    scene = mcpt.Scene(mcpt.ObjModel(path))
    assert scene.info()["node_boxes"] == 1
    p = mcpt.RenderParams(width=W, height=W, spp=1024, spp_chunk=32)
    mk, uc = scene.render_unit_counters(p)
    mk = mk.reshape(W, W, 3)
    wf, _ = scene.render(mcpt.RenderParams(width=W, height=W, spp=1024, spp_chunk=32, pipeline="wavefront"))
    region = (352, 592, 384, 624)
    x0, y0, x1, y1 = region
    ref, rc = oracle_mod.Scene(path).render(oracle_mod.RenderParams(
        width=W, height=W, spp=1024, spp_chunk=32, traversal=oracle_mod.KD_ORDERED, threads=_host_threads(),
        region=region, node_boxes=1))
    want = ref[y0:y1, x0:x1]
    for name, img in (("mega", mk), ("wave", wf)):
        assert np.array_equal(img[y0:y1, x0:x1].view(np.uint32), want.view(np.uint32)), name
    cc = _crop_counters(uc, _unit_order(mcpt, W, W), W * W, region, W)
    assert [int(x) for x in cc] == [rc["rays"], rc["inner_visits"], rc["leaf_visits"], rc["tri_tests"]]


def test_c5_full_spp_crop_matches_oracle(mcpt, oracle_mod, scene01):
    """BASELINE configs[4] (4096 spp, 128 chunks; the wavefront's batches span
    several chunks) on one GPU: a 64x64 crop over the glass sphere of the
    wavefront's, the material-sorted wavefront's and the megakernel's whole frames
    equals the oracle bit for bit."""
    W = 1024
    region = (608, 672, 672, 736)
    x0, y0, x1, y1 = region
    ref, _ = oracle_mod.Scene(mcpt.scene_path("scene01")).render(oracle_mod.RenderParams(
        width=W, height=W, spp=4096, spp_chunk=32, traversal=oracle_mod.KD_ORDERED, threads=_host_threads(),
        region=region))
    want = ref[y0:y1, x0:x1]
    for pipe, sort in (("wavefront", False), ("megakernel", False), ("wavefront", True)):
        img, st = scene01.render(mcpt.RenderParams(width=W, height=W, spp=4096, spp_chunk=32, pipeline=pipe, wf_sort=sort))
        assert st["rays"] > 1.3e10
        assert np.array_equal(img[y0:y1, x0:x1].view(np.uint32), want.view(np.uint32)), (pipe, sort)


def test_c5_wavefront_equals_megakernel_and_is_deterministic(mcpt, scene01):
    """C5 (1024x1024 @ 4096 spp, BASELINE configs[4]) on one GPU: the wavefront
    pipeline (its batches span several 32-sample chunks) renders the
    megakernel's frame bit for bit with equal counters, and twice the same."""
    import torch
    W = H = 1024
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, pipeline in (("mega", "megakernel"), ("wave", "wavefront"), ("wave2", "wavefront")):
        p = mcpt.RenderParams(width=W, height=H, spp=4096, spp_chunk=32, pipeline=pipeline)
        fb = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
        scene01.render_device(p, fb.data_ptr(), stream)
        torch.cuda.synchronize()
        out[name] = (fb, scene01.stats())
    ref, rs = out["mega"]
    assert rs["rays"] > 1.3e10
    for name in ("wave", "wave2"):
        img, st = out[name]
        assert torch.equal(img[:, :3], ref[:, :3]), name
        for k in ("rays", "paths", "inner_visits", "leaf_visits", "tri_tests", "shades"):
            assert st[k] == rs[k], (name, k, st[k], rs[k])
    # C5's split (BASELINE configs[4]: 4096 spp on 8 GPUs): the 8 packed
    # wavefront shards one rank each renders (lean, as bench.py times them)
    # reassemble the whole frame bit for bit, with the frame's rays
    N = 8
    got = torch.full((H * W, 4), -1.0, dtype=torch.float32, device="cuda")
    rays = 0
    for r in range(N):
        ps = mcpt.RenderParams(width=W, height=H, spp=4096, spp_chunk=32, shard_count=N, shard_index=r,
                               packed=True, tile=8, pipeline="wavefront", lean=True)
        part = torch.zeros((ps.output_pixels(), 4), dtype=torch.float32, device="cuda")
        scene01.render_device(ps, part.data_ptr(), stream)
        torch.cuda.synchronize()
        rays += scene01.stats()["rays"]
        xy = torch.from_numpy(ps.shard_pixels().astype(np.int64)).cuda()
        ok = xy[:, 0] >= 0
        got[(xy[:, 1] * W + xy[:, 0])[ok]] = part[ok]
    torch.cuda.synchronize()
    assert torch.equal(got[:, :3], ref[:, :3])
    assert rays == rs["rays"]


def test_progressive_render_matches_reference_image(mcpt):
    from PIL import Image
    ref = np.asarray(Image.open(os.path.join(GOLDEN, "result1.png")).convert("RGB")).astype(np.float32) / 255
    tr = mcpt.Tracer()
    tr.initialize([0])
    tr.create_geometry(mcpt.ObjModel(mcpt.scene_path("scene01")))
    host = np.zeros((600, 800, 3), np.float32)
    tr.render_scene(1, host, num_kernels=10, samples_per_kernel=100, illum=30.0, fresnel_kd=False)
    tr.destroy_geometry()
    enc = mcpt.encode_8bit(host).astype(np.float32) / 255
    blocks = lambda a: a.reshape(6, 100, 8, 100, 3).mean(axis=(1, 3))
    unsat = ~(ref >= 254 / 255).reshape(6, 100, 8, 100, 3).any(axis=(1, 3, 4))
    d = np.abs(blocks(host) - blocks(ref))[unsat]
    assert d.mean() < 0.003 and d.max() < 0.03, (d.mean(), d.max())
    rmse = float(np.sqrt(np.mean((enc - ref) ** 2)))
    # per-pixel: both images carry 1000-spp Monte Carlo noise (the reference's own
    # 100-vs-1000 spp RMSE is 0.031); the block means above carry the bias test
    assert rmse < 0.05, rmse


def test_progressive_ladder_matches_reference_steps(mcpt):
    """RenderScene's progressive loop pinned at every step, not only the last:
    after launch k (k+1 x 100 spp, prevCount = k, CUTracer.cu:215-217, 378-395)
    the 8-bit encode of the running mean matches the reference's own
    result1step/step00000k.png (800x600, the published variant: luminance 30,
    untinted Fresnel) on 50x50-pixel block means (8-bit units, blocks without a
    saturated pixel in any step), within a bias floor plus the Monte Carlo
    noise of both renders, which falls as 1/sqrt(k+1).  Thresholds from
    scripts/ladder_stats.py (the oracle renders this ladder bit-identically:
    per step mean |d| 0.33 .. 0.13, max 4.8 .. 0.9, mean d within +-0.03)."""
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    from ladder import ladder_stats
    g = np.load(os.path.join(GOLDEN, "result1step_blocks.npz"))
    tr = mcpt.Tracer()
    tr.initialize([0])
    tr.create_geometry(mcpt.ObjModel(mcpt.scene_path("scene01")))
    host = np.zeros((600, 800, 3), np.float32)
    stats = []
    tr.render_scene(1, host, num_kernels=10, samples_per_kernel=100, illum=30.0, fresnel_kd=False,
                    callback=lambda k, img: stats.append(ladder_stats(mcpt.encode_8bit(img), g, k)))
    tr.destroy_geometry()
    assert len(stats) == 10
    for k, (mean, mx, bias) in enumerate(stats):
        noise = 1.0 / np.sqrt(k + 1)
        assert mean < 0.08 + 0.32 * noise, (k, mean)
        assert mx < 0.8 + 5.0 * noise, (k, mx)
        assert abs(bias) < 0.06, (k, bias)
    assert stats[9][0] < 0.6 * stats[0][0]          # the noise falls along the ladder


def test_scene02_progressive_render_matches_mcdocx_figure3(mcpt):
    """scene02 (four spherical emitters, glossy slabs Ns 5/10/20/50, served from
    global memory with the child-box cull) through RenderScene(2)'s loop, 10 x
    100 spp at 800x600, luminance 10: its 75x75 block means match the
    reference's MC.docx Figure 3 (Blinn-Phong, luminance 10, 10000 spp), and the
    Phong-model render of Figure 4 / result2step/step000009.png is rejected
    (tests/test_brute_pins.py explains the two figures)."""
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    from test_brute_pins import _blocks_vs_figure, load_png
    tr = mcpt.Tracer()
    tr.initialize([0])
    tr.create_geometry(mcpt.ObjModel(mcpt.scene_path("scene02")))
    host = np.zeros((600, 800, 3), np.float32)
    tr.render_scene(2, host, num_kernels=10, samples_per_kernel=100, illum=10.0)
    tr.destroy_geometry()
    d3 = _blocks_vs_figure(host, load_png("mcdocx_fig3_scene2_blinn_phong.png"))
    assert d3.size >= 30 and d3.mean() < 0.006 and d3.max() < 0.010, (d3.mean(), d3.max())
    d4 = _blocks_vs_figure(host, load_png("mcdocx_fig4_scene2_phong.png"))
    assert d4.max() > 0.025, d4.max()
    step = load_png("result2_step000009.png")
    blocks = lambda a: a.reshape(6, 100, 8, 100, 3).mean(axis=(1, 3))  # noqa: E731
    assert np.abs(blocks(host) - blocks(step)).max() > 0.1
