"""Adaptive sampling on the wavefront pipeline (mcpt_render_adaptive_ex with
pipeline = "wavefront": wf_generate_list and the explicit queue 0 of
csrc/wavefront.hip under the selection, compaction and merge of
csrc/adaptive.hip), bit for bit against two references: (a) the numpy selection
(tests/_adaptive_ref.py) applied to the GPU's uniform `render_var` chain, and
(b) the megakernel's `render_adaptive` of the same params.  The work counters
are checked against the per-unit counters of each uniform pass, summed over
(pass j, pixel with count > j).  The helpers and the cached chains are those of
tests/test_gpu_adaptive.py.
"""
import numpy as np
import pytest

import test_gpu_adaptive as GA

pytestmark = pytest.mark.gpu

MAIN = GA.MAIN
TRAVERSAL = ("inner_visits", "leaf_visits", "leaf_refs", "tri_tests")
_unit = {}


def _adaptive(mcpt, passes, ap):
    return mcpt.adaptive_params(max_passes=passes, min_passes=ap.get("min_passes", 0), threshold=ap["threshold"],
                                lum_floor=ap.get("lum_floor", 0.0),
                                dilate={0: -1}.get(ap.get("dilate_r", 1), ap.get("dilate_r", 1)),
                                force_list=ap.get("force_list", False))


def _params(mcpt, W, H, S, chunk, **kw):
    return mcpt.RenderParams(width=W, height=H, spp=S, spp_chunk=chunk, **kw)


def _run_wf(mcpt, scene, W, H, S, chunk, passes, ap, **kw):
    return scene.render_adaptive_ex(_params(mcpt, W, H, S, chunk, pipeline="wavefront", **kw),
                                    _adaptive(mcpt, passes, ap))


def _run_mk(mcpt, scene, W, H, S, chunk, passes, ap, **kw):
    return scene.render_adaptive(_params(mcpt, W, H, S, chunk, **kw), _adaptive(mcpt, passes, ap))


def _pass_counters(mcpt, W, H, S, chunk, passes, tile=8, spp_offset=0, **fields):
    """(passes, H, W, 4) uint64: rays, inner, leaf, tests of every pixel in every uniform pass, from
    the megakernel's render_unit_counters (any frame: units of tile padding own no pixel)"""
    key = (W, H, S, chunk, passes, tile, spp_offset, tuple(sorted(fields.items())))
    if key not in _unit:
        inv, nch = GA._unit_order(mcpt, W, H, tile), (S + chunk - 1) // chunk
        npk = GA._packed_count(mcpt, W, H, tile)
        assert (inv >= 0).all()
        out = np.zeros((passes, H * W, 4), np.uint64)
        for j in range(passes):
            _, uc = GA._scene(mcpt).render_unit_counters(_params(mcpt, W, H, S, chunk, spp_offset=spp_offset + j * S,
                                                                 tile=tile, **fields))
            assert uc.shape == (npk * nch, 4)
            out[j] = uc.reshape(nch, npk, 4).astype(np.uint64).sum(axis=0)[inv]
        _unit[key] = out.reshape(passes, H, W, 4)
    return _unit[key]


def _check(mcpt, got, ref, mk, frame, lean, variant=4, traversal=True, **counter_kw):
    """got against (a) ref = (chain, fb, var, count) and (b) mk, the megakernel's adaptive render"""
    fb, var, count, st = got
    S = frame["S"]
    print("count histogram", np.bincount(count.ravel()).tolist(), "stats", st)
    GA._check_images(got, ref, S)
    GA._assert_equal(fb, mk[0], "framebuffer against the megakernel's")
    GA._assert_equal(var, mk[1], "variance against the megakernel's")
    assert np.array_equal(count, mk[2])
    assert st["variant"] == variant
    # (a lean megakernel render counts nothing: paths and rays are then the chain's and the unit counters')
    for k in ("renders",) if lean else ("paths", "renders", "rays"):
        assert st[k] == mk[3][k], (k, st[k], mk[3][k])
    pc = _pass_counters(mcpt, frame["W"], frame["H"], S, frame["chunk"], frame["passes"], **counter_kw)
    want = np.zeros(4, np.uint64)
    for j in range(frame["passes"]):
        want += pc[j][ref[3] > j].sum(axis=0)
    print("unit counters summed", want.tolist())
    assert st["rays"] == int(want[0])
    if lean:
        assert all(st[k] == 0 for k in TRAVERSAL), st
    elif traversal:
        for i, k in ((1, "inner_visits"), (2, "leaf_visits"), (3, "tri_tests")):
            assert st[k] == int(want[i]), (k, st[k], int(want[i]))
        assert st["leaf_refs"] == mk[3]["leaf_refs"]


def _case(mcpt, frame, ap, lean, scene=None, variant=4, traversal=True, chain_kw=None, **kw):
    """one wavefront adaptive render of `frame` checked against both references; kw: render
    params; chain_kw: those of them that change the image (the chain's and the counters' too)"""
    chain_kw = chain_kw or {}
    scene = scene or GA._scene(mcpt)
    ref = GA._reference(mcpt, **frame, ap=ap, **chain_kw)
    mk = _run_mk(mcpt, scene, **frame, ap=ap, lean=lean, **chain_kw, **kw)
    got = _run_wf(mcpt, scene, **frame, ap=ap, lean=lean, **chain_kw, **kw)
    ckw = dict(chain_kw)
    if "tile" in kw:
        ckw["tile"] = kw["tile"]
    _check(mcpt, got, ref, mk, frame, lean, variant=variant, traversal=traversal, **ckw)
    return got, ref


# ---- 1. the main frame ------------------------------------------------------------

@pytest.mark.parametrize("lean", [True, False], ids=["lean", "counting"])
@pytest.mark.parametrize("dilate_r,hist", [(1, [1202, 42, 41, 31, 7, 45, 42, 1662]),
                                           (0, [2710, 36, 30, 19, 9, 25, 16, 227])], ids=["dilate-1", "no-dilation"])
def test_main_frame_equals_the_chain_and_the_megakernel(mcpt, dilate_r, hist, lean):
    ap = dict(threshold=0.5, dilate_r=dilate_r)
    got, ref = _case(mcpt, MAIN, ap, lean)
    assert np.bincount(ref[3].ravel(), minlength=9)[1:].tolist() == hist          # every count 1..8 occurs


# ---- 2. short lists ---------------------------------------------------------------

@pytest.mark.parametrize("threshold,listed", [(0.97, [83, 4, 1]), (0.95, [135, 65, 2]), (0.98, [5])],
                         ids=["one-pixel", "wave-and-one", "sub-wave"])
def test_short_lists(mcpt, threshold, listed):
    """a one-pixel pass (every segment but one empty), passes of less than a wave, a pass of 65..127"""
    ap = dict(threshold=threshold, dilate_r=0)
    ref = GA._reference(mcpt, **MAIN, ap=ap)
    sizes = [n for n in GA._list_sizes(ref[0], MAIN["passes"], ap) if n]
    print("threshold", threshold, "listed", sizes)
    assert sizes[:len(listed)] == listed                  # (the first lists of the reference, as the oracle has them)
    assert {0.97: 1 in sizes, 0.95: any(65 <= n <= 127 for n in sizes), 0.98: any(2 <= n <= 63 for n in sizes)}[threshold]
    _case(mcpt, MAIN, ap, True)


# ---- 3. batch splits of a listed pass, streams, refill ------------------------------

@pytest.mark.parametrize("kw,passes", [(dict(wf_batch=1000), 8), (dict(wf_batch=2), 3), (dict(wf_streams=1), 8),
                                       (dict(wf_streams=3), 8), (dict(wf_streams=4), 8), (dict(wf_refill=1), 8),
                                       (dict(wf_refill=64), 8)],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_batch_splits_streams_and_refill(mcpt, kw, passes):
    """wf_batch = 1000: 64-path groups straddle samples and a batch cuts the list mid-tile;
    wf_batch = 2, the chunk: one listed pixel per batch"""
    frame = dict(MAIN, passes=passes)
    ap = dict(threshold=0.5)
    got, ref = _case(mcpt, frame, ap, True, **kw)
    assert ref[3].max() == passes and (np.bincount(ref[3].ravel()) > 0).sum() >= 3


# ---- 4. chunking ------------------------------------------------------------------

@pytest.mark.parametrize("S,chunk", [(15, 7), (10, 3)])
def test_partial_last_chunks(mcpt, S, chunk):
    frame = dict(W=37, H=29, S=S, chunk=chunk, passes=4)
    ap = dict(threshold=0.5)
    got, ref = _case(mcpt, frame, ap, False)
    hist = np.bincount(ref[3].ravel(), minlength=5)
    assert (hist > 0).sum() >= 2 and hist[4] > 0, hist.tolist()


def test_sample_offset_and_seed(mcpt):
    ap = dict(threshold=0.5)
    got, ref = _case(mcpt, MAIN, ap, False, chain_kw=dict(spp_offset=1000, seed=12345))
    assert not np.array_equal(ref[3], GA._reference(mcpt, **MAIN, ap=ap)[3])
    assert (np.bincount(ref[3].ravel()) > 0).sum() >= 3


# ---- 5. tiles ---------------------------------------------------------------------

@pytest.mark.parametrize("tile,W,H", [(4, 36, 28), (16, 37, 29)])
def test_other_tile_sizes(mcpt, tile, W, H):
    """the list is in that tiling's packed order"""
    frame = dict(W=W, H=H, S=8, chunk=2, passes=4)
    ap = dict(threshold=0.5)
    got, ref = _case(mcpt, frame, ap, False, tile=tile)
    sizes = GA._list_sizes(ref[0], 4, ap)
    assert len(sizes) == 3 and all(0 < n < W * H for n in sizes), sizes


# ---- 6. force_list ------------------------------------------------------------------

@pytest.mark.parametrize("tile,W,H,fields", [(8, 64, 48, {}), (8, 8, 8, {}), (1, 9, 7, {}), (1, 13, 5, {}),
                                             (8, 1, 1, dict(spp_offset=48))],
                         ids=lambda v: str(v) if not isinstance(v, dict) else "-".join(f"{k}{x}" for k, x in v.items()))
def test_force_list_is_the_wavefront_chain(mcpt, tile, W, H, fields):
    """min_passes = max_passes = 3 through the list: the whole frame listed twice"""
    frame = dict(W=W, H=H, S=8, chunk=2, passes=3)
    ap = dict(threshold=0.5, min_passes=3, force_list=True)
    scene = GA._scene(mcpt)
    fb = var = None
    for j in range(3):       # the wavefront's own uniform chain
        fb, var, _ = scene.render_var(_params(mcpt, W, H, 8, 2, pipeline="wavefront", lean=True, tile=tile,
                                              prev_count=j, spp_offset=fields.get("spp_offset", 0) + 8 * j), fb, var)
    got, ref = _case(mcpt, frame, ap, True, chain_kw=fields, tile=tile)
    assert (got[2] == 3).all()
    assert got[1][..., :3].max() > 0
    GA._assert_equal(got[0], fb, "framebuffer against the wavefront chain")
    GA._assert_equal(got[1], var, "variance against the wavefront chain")
    assert got[3]["paths"] == 3 * 8 * W * H and got[3]["renders"] == 3


# ---- 7. depths ----------------------------------------------------------------------

@pytest.mark.parametrize("max_depth", [0, 1])
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "counting"])
def test_depths_0_and_1(mcpt, max_depth, lean):
    """max_depth = 0: the generated ray is itself the terminal query"""
    frame = dict(W=32, H=24, S=8, chunk=2, passes=3)
    ap = dict(threshold=0.95, dilate_r=0)
    got, ref = _case(mcpt, frame, ap, lean, chain_kw=dict(max_depth=max_depth))
    sizes = GA._list_sizes(ref[0], 3, ap)
    print("max_depth", max_depth, "listed", sizes)
    assert sizes and sizes[0] > 0 and got[3]["renders"] >= 2          # a listed pass ran


# ---- 8. material sort -----------------------------------------------------------------

@pytest.mark.parametrize("lean", [True, False], ids=["lean", "counting"])
def test_material_sort(mcpt, lean):
    _case(mcpt, MAIN, dict(threshold=0.5), lean, wf_sort=True)


# ---- 9. global layout -----------------------------------------------------------------

@pytest.mark.parametrize("lean", [True, False], ids=["lean", "counting"])
@pytest.mark.parametrize("shift", [0, 6])
def test_global_layout(mcpt, shift, lean):
    scene = GA._scene(mcpt, "global")
    assert int(scene.info()["node_boxes"]) == 1
    ap = dict(threshold=0.5)
    ref = GA._reference(mcpt, **MAIN, ap=ap)
    mk = _run_mk(mcpt, scene, **MAIN, ap=ap, lean=lean)
    got = _run_wf(mcpt, scene, **MAIN, ap=ap, lean=lean, wf_group_shift=shift)
    # (the unit counters are the LDS layout's walk; the global layout's, with its child-box
    # cull, is compared with the megakernel's render of the same scene)
    _check(mcpt, got, ref, mk, MAIN, lean, variant=5, traversal=False)
    if not lean:
        for k in TRAVERSAL:
            assert got[3][k] == mk[3][k], (k, got[3][k], mk[3][k])


# ---- 10. the culls stay on in listed passes ---------------------------------------------

def test_culls_stay_on_in_listed_passes(mcpt):
    scene = GA._scene(mcpt)
    fb, var, count, st = _run_wf(mcpt, scene, **MAIN, ap=dict(threshold=0.5), lean=True)
    print(st)
    assert st["direct_rays"] > 0
    assert st["extend_rays"] + st["direct_rays"] <= st["rays"] - st["paths"]
    # per pass: the direct test depends on the ray alone, not on the kernel that made the primary ray
    frame = dict(MAIN, passes=2)
    got = _run_wf(mcpt, scene, **frame, ap=dict(threshold=0.5, min_passes=2, force_list=True), lean=True)
    uni = [scene.render_var(_params(mcpt, 64, 48, 8, 2, pipeline="wavefront", lean=True, spp_offset=8 * j))[2]
           for j in range(2)]
    print(got[3], uni)
    assert uni[0]["direct_rays"] > 0 and uni[1]["direct_rays"] > 0
    assert got[3]["direct_rays"] == uni[0]["direct_rays"] + uni[1]["direct_rays"]
    assert got[3]["rays"] == uni[0]["rays"] + uni[1]["rays"]
    # the listed pass shades bounce 0 in the shade kernel: only pass 0's paths were eligible
    assert got[3]["primary_shaded"] == uni[0]["primary_shaded"]


# ---- 11. device and host entries ----------------------------------------------------------

def test_device_entry_equals_host_entry_and_allocates_nothing(mcpt):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    p = _params(mcpt, 64, 48, 8, 2, pipeline="wavefront", lean=True)
    a = mcpt.adaptive_params(threshold=0.5)
    d_fb = torch.full((p.height, p.width, 4), -1.0, device="cuda")
    d_var = torch.full((p.height, p.width, 4), -1.0, device="cuda")
    d_cnt = torch.full((p.height, p.width), -1, dtype=torch.int32, device="cuda")
    ptrs = (d_fb.data_ptr(), d_var.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    scene.reserve(p)
    scene.render_adaptive_ex_device(p, a, *ptrs)
    torch.cuda.synchronize()
    first = [t.cpu().numpy().copy() for t in (d_fb, d_var, d_cnt)]
    st_first = scene.stats()                                            # (its timing events return to the pool)
    for t in (d_fb, d_var):
        t.fill_(-1.0)
    d_cnt.fill_(-1)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    scene.render_adaptive_ex_device(p, a, *ptrs)                        # no allocation
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    st_dev = scene.stats()
    fb, var, count, st = scene.render_adaptive_ex(p, a)
    ref = GA._reference(mcpt, **MAIN, ap=dict(threshold=0.5))
    assert np.array_equal(count, ref[3]) and count.max() == 8
    for got in (first, [t.cpu().numpy() for t in (d_fb, d_var, d_cnt)]):
        GA._assert_equal(got[0][..., :3], fb, "device vs host framebuffer")
        assert (got[0][..., 3] == 0).all()
        GA._assert_equal(got[1], var, "device vs host variance")
        assert np.array_equal(got[2].astype(np.uint32), count)
    for k in GA.INT_STATS + ("direct_rays", "extend_rays", "clipped_rays", "primary_shaded"):
        assert st_first[k] == st_dev[k] == st[k], k
    assert st["variant"] == 4


# ---- 12. later renders and early exits ------------------------------------------------------

def test_later_renders_tile_classes_and_early_exits(mcpt):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    W, H = 64, 48
    mk = _params(mcpt, W, H, 8, 2)
    wf = _params(mcpt, W, H, 8, 2, pipeline="wavefront", lean=True)
    before = [scene.render(q) for q in (mk, wf)]
    tc = scene.primary_tile_classes()
    assert tc["empty"] + tc["listed"] + tc["walked"] == (W // 8) * (H // 8)      # the uniform render used the lists
    fb, var, count, st = scene.render_adaptive_ex(wf, mcpt.adaptive_params(threshold=0.5))
    assert count.max() == 8 and count.min() == 1 and st["variant"] == 4
    # the last pass was listed: no tile classes, as after any render that did not use the lists
    tc = scene.primary_tile_classes()
    assert (tc["empty"], tc["listed"], tc["walked"]) == (0, 0, 0), tc
    for q, (rfb, rst) in zip((mk, wf), before):
        fb2, st2 = scene.render(q)
        GA._assert_equal(fb2, rfb, "render after render_adaptive_ex")
        assert st2["renders"] == 1 and st2["rays"] == rst["rays"] and st2["paths"] == rst["paths"]
    tc = scene.primary_tile_classes()
    assert tc["empty"] + tc["listed"] + tc["walked"] == (W // 8) * (H // 8)
    # one pass is the wavefront's render_var
    p = _params(mcpt, 37, 29, 8, 2, pipeline="wavefront", lean=True)
    rfb, rvar, rst = scene.render_var(p)
    fb, var, count, st = scene.render_adaptive_ex(p, mcpt.adaptive_params(max_passes=1))
    GA._assert_equal(fb, rfb, "framebuffer")
    GA._assert_equal(var, rvar, "variance")
    assert (count == 1).all() and count.shape == (29, 37)
    assert {k: st[k] for k in GA.INT_STATS} == {k: rst[k] for k in GA.INT_STATS}
    # a huge threshold ends after pass 0
    fb, var, count, st = scene.render_adaptive_ex(wf, mcpt.adaptive_params(threshold=1e30))
    chain = GA._chain(mcpt, W, H, 8, 2, 1)
    GA._assert_equal(fb, chain[0][0], "framebuffer")
    GA._assert_equal(var, chain[0][1], "variance")
    assert (count == 1).all() and st["renders"] == 1 and st["paths"] == 8 * W * H and st["variant"] == 4
    tc = scene.primary_tile_classes()                                    # pass 0, a uniform render, was the last
    assert tc["empty"] + tc["listed"] + tc["walked"] == (W // 8) * (H // 8)


# ---- 13. refusals launch nothing ---------------------------------------------------------------

def test_ex_refusals_launch_nothing(mcpt):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    W, H = 32, 24
    d_fb = torch.full((H, W, 4), -1.0, device="cuda")
    d_var = torch.full((H, W, 4), -1.0, device="cuda")
    d_cnt = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    scene.stats()
    ptrs = (d_fb.data_ptr(), d_var.data_ptr(), d_cnt.data_ptr())
    P = lambda **kw: mcpt.RenderParams(**{**dict(width=W, height=H, spp=4, spp_chunk=2,   # noqa: E731
                                                 pipeline="wavefront"), **kw})
    cases = [(P(spp_chunk=0), None, -1), (P(prev_count=2), None, -1), (P(spp_offset=2 ** 32 - 8), None, -1),
             (P(), mcpt.adaptive_params(max_passes=5000), -1), (P(), mcpt.adaptive_params(min_passes=9), -1),
             (P(), mcpt.adaptive_params(threshold=-1.0), -1), (P(), mcpt.adaptive_params(lum_floor=-1.0), -1),
             (P(), mcpt.adaptive_params(dilate=5), -1),
             (P(shard_count=2), None, -6), (P(packed=True), None, -6), (P(gather="rccl"), None, -6),
             (mcpt.RenderParams.for_quinengine(width=W, height=H, spp=4, spp_chunk=2, pipeline="wavefront"), None, -6)]
    for p, a, code in cases:
        with pytest.raises(mcpt.McptError) as e:
            scene.render_adaptive_ex_device(p, a, *ptrs)
        assert e.value.code == code, (code, str(e.value))
        with pytest.raises(mcpt.McptError) as e:
            scene.render_adaptive_ex(p, a)
        assert e.value.code == code, (code, str(e.value))
    with pytest.raises(mcpt.McptError) as e:
        scene.render_adaptive_ex_device(P(), None, ptrs[0], ptrs[0] + 16, ptrs[2])
    assert e.value.code == -1 and "overlap" in str(e.value)
    # a capturing stream: refused, nothing captured
    scene.reserve(P())
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        try:
            scene.render_adaptive_ex_device(P(), None, *ptrs, s.cuda_stream)
        except mcpt.McptError as e:
            err = e
        d_cnt.add_(1)    # (the graph is not empty)
    assert err is not None and err.code == -6 and "capturing" in str(err), err
    d_cnt.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert bool((d_cnt == 0).all())
    assert bool((d_fb == -1.0).all()) and bool((d_var == -1.0).all())
    st = scene.stats()
    assert st["renders"] == 0 and st["rays"] == 0 and st["paths"] == 0


# ---- 14. the general form on the megakernel ------------------------------------------------------

def test_ex_on_the_megakernel_is_render_adaptive(mcpt):
    scene = GA._scene(mcpt)
    ap = dict(threshold=0.5)
    mk = _run_mk(mcpt, scene, **MAIN, ap=ap)
    ex = scene.render_adaptive_ex(_params(mcpt, 64, 48, 8, 2, pipeline="megakernel"), _adaptive(mcpt, 8, ap))
    GA._assert_equal(ex[0], mk[0], "framebuffer")
    GA._assert_equal(ex[1], mk[1], "variance")
    assert np.array_equal(ex[2], mk[2]) and ex[2].max() == 8
    assert {k: ex[3][k] for k in GA.INT_STATS} == {k: mk[3][k] for k in GA.INT_STATS}
