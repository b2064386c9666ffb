"""Variance-driven adaptive sampling on the GPU (mcpt_render_adaptive: the
pixel-list megakernel of csrc/render.hip, the selection, compaction and merge
kernels of csrc/adaptive.hip), bit for bit against the GPU's own uniform chain:
`render_var` with prev_count = j and spp_offset = j S saved after each pass,
the numpy selection (tests/_adaptive_ref.py) applied to those images, and the
per-unit counters of each uniform pass for the work counters.
"""
import numpy as np
import pytest

import _adaptive_ref as AR

pytestmark = pytest.mark.gpu

_scenes = {}
_chains = {}
_counters = {}
INT_STATS = ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades", "stack_spills",
             "renders", "variant", "devices")


def _scene(mcpt, layout="auto"):
    if layout not in _scenes:
        _scenes[layout] = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), layout=layout)
    return _scenes[layout]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equal(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(),
                           got[bad][:5].tolist(), ref[bad][:5].tolist())


def _chain(mcpt, W, H, S, chunk, passes):
    """[(fb, var) after j + 1 chained uniform render_var calls], computed once per frame and
    left unchanged (a longer chain of the same frame serves the shorter ones)"""
    key = (W, H, S, chunk)
    have = _chains.setdefault(key, [])
    scene = _scene(mcpt)
    while len(have) < passes:
        j = len(have)
        fb, var = (have[-1][0].copy(), have[-1][1].copy()) if j else (None, None)
        fb, var, _ = scene.render_var(mcpt.RenderParams(width=W, height=H, spp=S, spp_chunk=chunk, spp_offset=j * S,
                                                        prev_count=j), fb, var)
        fb.setflags(write=False)
        var.setflags(write=False)
        have.append((fb, var))
    return have[:passes]


def _unit_order(mcpt, W, H, tile=8):
    """row-major pixel index -> work-unit pixel index v (tile-major, render.hip unit_pixel)"""
    xy = mcpt.RenderParams(width=W, height=H, tile=tile, packed=True).shard_pixels()
    inv = np.full(W * H, -1, np.int64)
    ok = xy[:, 0] >= 0
    inv[xy[ok, 1] * W + xy[ok, 0]] = np.nonzero(ok)[0]
    return inv


def _pass_counters(mcpt, W, H, S, chunk, passes):
    """(passes, H, W, 4) uint64: rays, inner, leaf, tests of every pixel in every uniform pass
    (summed over the pass's chunks), from render_unit_counters; W and H multiples of the tile"""
    key = (W, H, S, chunk, passes)
    if key not in _counters:
        assert W % 8 == 0 and H % 8 == 0
        inv, npix, nch = _unit_order(mcpt, W, H), W * H, (S + chunk - 1) // chunk
        out = np.zeros((passes, H * W, 4), np.uint64)
        for j in range(passes):
            _, uc = _scene(mcpt).render_unit_counters(mcpt.RenderParams(width=W, height=H, spp=S, spp_chunk=chunk,
                                                                        spp_offset=j * S))
            assert uc.shape == (npix * nch, 4)
            out[j] = uc.reshape(nch, npix, 4).astype(np.uint64).sum(axis=0)[inv]
        _counters[key] = out.reshape(passes, H, W, 4)
    return _counters[key]


def _reference(mcpt, W, H, S, chunk, passes, ap):
    chain = _chain(mcpt, W, H, S, chunk, passes)
    fb, var, count, _ = AR.adaptive_from_chain(chain, max_passes=passes, min_passes=ap.get("min_passes", 1),
                                               threshold=ap["threshold"], lum_floor=ap.get("lum_floor", 0.01),
                                               dilate_r=ap.get("dilate_r", 1))
    return chain, fb, var, count


def _run(mcpt, scene, W, H, S, chunk, passes, ap, **kw):
    a = mcpt.adaptive_params(max_passes=passes, min_passes=ap.get("min_passes", 0), threshold=ap["threshold"],
                             lum_floor=ap.get("lum_floor", 0.0), dilate={0: -1}.get(ap.get("dilate_r", 1),
                                                                                     ap.get("dilate_r", 1)),
                             force_list=ap.get("force_list", False))
    return scene.render_adaptive(mcpt.RenderParams(width=W, height=H, spp=S, spp_chunk=chunk, **kw), a)


def _check_images(got, ref, S):
    fb, var, count, st = got
    chain, rfb, rvar, rcount = ref
    assert count.dtype == np.uint32 and np.array_equal(count, rcount), \
        (np.bincount(count.ravel()).tolist(), np.bincount(rcount.ravel()).tolist())
    for m in np.unique(rcount):
        sel = rcount == m
        _assert_equal(fb[sel], chain[m - 1][0][sel], f"fb of count {m}")
        _assert_equal(var[sel], chain[m - 1][1][sel], f"var of count {m}")
    _assert_equal(fb, rfb, "framebuffer")
    _assert_equal(var, rvar, "variance")
    assert (var[..., 3] == 0).all()
    assert st["paths"] == S * int(rcount.astype(np.uint64).sum())
    assert st["renders"] == int(rcount.max())


def _check_counters(mcpt, st, rcount, W, H, S, chunk, passes, names=("rays", "inner_visits", "leaf_visits",
                                                                     "tri_tests")):
    pc = _pass_counters(mcpt, W, H, S, chunk, passes)
    want = np.zeros(4, np.uint64)
    for j in range(passes):
        want += pc[j][rcount > j].sum(axis=0)
    for i, k in enumerate(("rays", "inner_visits", "leaf_visits", "tri_tests")):
        if k in names:
            assert st[k] == int(want[i]), (k, st[k], int(want[i]))


MAIN = dict(W=64, H=48, S=8, chunk=2, passes=8)


def _covered(rcount):
    """the reference exercises the list: three pass counts with >= 16 pixels each, and both ends"""
    hist = np.bincount(rcount.ravel(), minlength=9)
    assert int((hist >= 16).sum()) >= 3, hist.tolist()
    assert hist[1] > 0 and hist[8] > 0, hist.tolist()


@pytest.mark.parametrize("dilate_r", [1, 0], ids=["dilate-1", "no-dilation"])
def test_adaptive_equals_the_uniform_chain_per_pixel(mcpt, dilate_r):
    ap = dict(threshold=0.5, dilate_r=dilate_r)
    ref = _reference(mcpt, **MAIN, ap=ap)
    _covered(ref[3])
    got = _run(mcpt, _scene(mcpt), **MAIN, ap=ap)
    print("count histogram", np.bincount(got[2].ravel()).tolist(), "stats", got[3])
    _check_images(got, ref, MAIN["S"])
    _check_counters(mcpt, got[3], ref[3], **MAIN)


VARIANTS = [
    # id, frame, adaptive params, scene layout, render params, counters compared
    ("no-tail-split", MAIN, dict(threshold=0.5), "auto", dict(tail_units_per_lane=-1), True),
    ("mixed-tail-500", MAIN, dict(threshold=0.5), "auto", dict(tail_units=500), True),   # both kinds of unit listed
    ("global-layout", MAIN, dict(threshold=0.5), "global", {}, False),
    ("ragged-37x29", dict(W=37, H=29, S=12, chunk=4, passes=4), dict(threshold=0.5), "auto", {}, False),
    ("short-last-chunk", dict(W=64, H=48, S=10, chunk=4, passes=4), dict(threshold=0.5), "auto", {}, False),
    ("more-pixels-than-lanes", dict(W=608, H=440, S=2, chunk=1, passes=3), dict(threshold=0.5), "auto", {}, False),
    ("min-passes-3", MAIN, dict(threshold=0.5, min_passes=3), "auto", {}, True),
]


@pytest.mark.parametrize("case", VARIANTS, ids=lambda c: c[0])
def test_adaptive_variants_equal_the_uniform_chain(mcpt, case):
    _, frame, ap, layout, kw, counters = case
    scene = _scene(mcpt, layout)
    if layout == "global":
        assert int(scene.info()["node_boxes"]) == 1
    ref = _reference(mcpt, **frame, ap=ap)
    hist = np.bincount(ref[3].ravel())
    assert (hist > 0).sum() >= 2, hist.tolist()                  # some pixels stop early, some go on
    if ap.get("min_passes"):
        assert ref[3].min() == ap["min_passes"]
    got = _run(mcpt, scene, **frame, ap=ap, **kw)
    _check_images(got, ref, frame["S"])
    if counters:
        _check_counters(mcpt, got[3], ref[3], **frame)


def test_adaptive_lean_gives_the_same_image_and_rays(mcpt):
    ap = dict(threshold=0.5)
    ref = _reference(mcpt, **MAIN, ap=ap)
    fb, var, count, st = _run(mcpt, _scene(mcpt), **MAIN, ap=ap, lean=True)
    assert np.array_equal(count, ref[3])
    _assert_equal(fb, ref[1], "framebuffer")
    _assert_equal(var, ref[2], "variance")
    _check_counters(mcpt, st, ref[3], **MAIN, names=("rays",))


def test_force_list_with_every_pixel_listed_is_the_uniform_chain(mcpt):
    """min_passes = max_passes = 3 through the list: the whole image in the list twice"""
    frame = dict(W=64, H=48, S=8, chunk=2, passes=3)
    chain = _chain(mcpt, 64, 48, 8, 2, 3)
    ap = dict(threshold=0.5, min_passes=3, force_list=True)
    fb, var, count, st = _run(mcpt, _scene(mcpt), **frame, ap=ap)
    assert (count == 3).all()
    _assert_equal(fb, chain[2][0], "framebuffer")
    _assert_equal(var, chain[2][1], "variance")
    _check_counters(mcpt, st, count, **frame)
    assert st["paths"] == 3 * 8 * 64 * 48 and st["renders"] == 3
    # and without the list: the same
    fb2, var2, count2, st2 = _run(mcpt, _scene(mcpt), **frame, ap=dict(threshold=0.5, min_passes=3))
    _assert_equal(fb2, fb, "framebuffer, full-frame passes")
    _assert_equal(var2, var, "variance, full-frame passes")
    assert (count2 == 3).all() and {k: st2[k] for k in INT_STATS} == {k: st[k] for k in INT_STATS}


# ---- edges ------------------------------------------------------------------------

def test_one_pass_is_render_var(mcpt):
    scene = _scene(mcpt)
    p = mcpt.RenderParams(width=37, height=29, spp=8, spp_chunk=2)
    rfb, rvar, rst = scene.render_var(p)
    fb, var, count, st = scene.render_adaptive(p, mcpt.adaptive_params(max_passes=1))
    _assert_equal(fb, rfb, "framebuffer")
    _assert_equal(var, rvar, "variance")
    assert (count == 1).all() and count.shape == (29, 37)
    assert {k: st[k] for k in INT_STATS} == {k: rst[k] for k in INT_STATS}


def test_a_huge_threshold_ends_after_pass_0(mcpt):
    scene = _scene(mcpt)
    p = mcpt.RenderParams(width=64, height=48, spp=8, spp_chunk=2)
    fb, var, count, st = scene.render_adaptive(p, mcpt.adaptive_params(threshold=1e30))
    chain = _chain(mcpt, 64, 48, 8, 2, 1)
    _assert_equal(fb, chain[0][0], "framebuffer")
    _assert_equal(var, chain[0][1], "variance")
    assert (count == 1).all() and st["renders"] == 1 and st["paths"] == 8 * 64 * 48


def test_host_and_device_entries_agree_without_allocation_or_side_effects(mcpt):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    p = mcpt.RenderParams(width=64, height=48, spp=8, spp_chunk=2)
    a = mcpt.adaptive_params(threshold=0.5)
    before, st0 = scene.render(p)
    d_fb = torch.full((p.height, p.width, 4), -1.0, device="cuda")
    d_var = torch.full((p.height, p.width, 4), -1.0, device="cuda")
    d_cnt = torch.full((p.height, p.width), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    scene.reserve(p)
    scene.render_adaptive_device(p, a, d_fb.data_ptr(), d_var.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    first = [t.cpu().numpy().copy() for t in (d_fb, d_var, d_cnt)]
    st_first = scene.stats()                                            # (its timing events return to the pool)
    free0 = scene.plan(p)["device_free_bytes"]
    for t in (d_fb, d_var):
        t.fill_(-1.0)
    d_cnt.fill_(-1)
    scene.render_adaptive_device(p, a, d_fb.data_ptr(), d_var.data_ptr(), d_cnt.data_ptr())   # no allocation
    torch.cuda.synchronize()
    assert scene.plan(p)["device_free_bytes"] == free0
    st_dev = scene.stats()
    fb, var, count, st = scene.render_adaptive(p, a)
    ref = _reference(mcpt, **MAIN, ap=dict(threshold=0.5))
    assert np.array_equal(count, ref[3])
    for got in (first, [t.cpu().numpy() for t in (d_fb, d_var, d_cnt)]):
        _assert_equal(got[0][..., :3], fb, "device vs host framebuffer")
        assert (got[0][..., 3] == 0).all()
        _assert_equal(got[1], var, "device vs host variance")
        assert np.array_equal(got[2].astype(np.uint32), count)
    for k in INT_STATS:
        assert st_first[k] == st_dev[k] == st[k], k
    after, st2 = scene.render(p)                                        # a later plain render: the same bits
    _assert_equal(after, before, "render after render_adaptive")
    assert st2["renders"] == 1 and st2["rays"] == st0["rays"]


def test_refusals_launch_nothing(mcpt):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    W, H = 32, 24
    d_fb = torch.full((H, W, 4), -1.0, device="cuda")
    d_var = torch.full((H, W, 4), -1.0, device="cuda")
    d_cnt = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    scene.stats()
    ptrs = (d_fb.data_ptr(), d_var.data_ptr(), d_cnt.data_ptr())
    P = lambda **kw: mcpt.RenderParams(**{**dict(width=W, height=H, spp=4, spp_chunk=2), **kw})   # noqa: E731
    cases = [(P(spp_chunk=0), None, -1), (P(prev_count=2), None, -1), (P(spp_offset=2 ** 32 - 8), None, -1),
             (P(), mcpt.adaptive_params(max_passes=5000), -1), (P(), mcpt.adaptive_params(min_passes=9), -1),
             (P(), mcpt.adaptive_params(threshold=-1.0), -1), (P(), mcpt.adaptive_params(lum_floor=-1.0), -1),
             (P(), mcpt.adaptive_params(dilate=5), -1),
             (P(shard_count=2), None, -6), (P(packed=True), None, -6), (P(gather="rccl"), None, -6),
             (P(pipeline="wavefront"), None, -6),
             (mcpt.RenderParams.for_quinengine(width=W, height=H, spp=4, spp_chunk=2), None, -6)]
    for p, a, code in cases:
        with pytest.raises(mcpt.McptError) as e:
            scene.render_adaptive_device(p, a, *ptrs)
        assert e.value.code == code, (code, str(e.value))
        with pytest.raises(mcpt.McptError) as e:
            scene.render_adaptive(p, a)
        assert e.value.code == code, (code, str(e.value))
    with pytest.raises(mcpt.McptError) as e:
        scene.render_adaptive_device(P(), None, ptrs[0], ptrs[0] + 16, ptrs[2])
    assert e.value.code == -1 and "overlap" in str(e.value)
    # a capturing stream: refused, nothing captured
    scene.reserve(P())
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        try:
            scene.render_adaptive_device(P(), None, *ptrs, s.cuda_stream)
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


# ---- the public pipeline ----------------------------------------------------------

def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_adaptive_reaches_the_error_of_six_uniform_passes_with_fewer_samples(mcpt):
    """tests/test_adaptive_cpu.py's assertion on the public entry (threshold 0.2, dilate 1, the
    defaults), against a converged 1024-spp GPU render of other samples."""
    scene = _scene(mcpt)
    W, H = 64, 48
    ref, _ = scene.render(mcpt.RenderParams(width=W, height=H, spp=1024, spp_offset=100000))
    fb, _, count, st = scene.render_adaptive(mcpt.RenderParams(width=W, height=H, spp=8, spp_chunk=2))
    chain = _chain(mcpt, W, H, 8, 2, 8)
    e, e6 = _rmse(fb, ref), _rmse(chain[5][0], ref)
    print(f"adaptive RMSE {e:.4f} at {count.mean():.2f} mean passes; uniform 6 / 7 / 8: {e6:.4f} / "
          f"{_rmse(chain[6][0], ref):.4f} / {_rmse(chain[7][0], ref):.4f}")
    assert float(count.mean()) <= 6.0
    assert e <= e6
