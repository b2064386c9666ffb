"""Variance-driven adaptive sampling on the GPU (mcpt_render_adaptive: the
pixel-list megakernel of csrc/render.hip, the selection, compaction and merge
kernels of csrc/adaptive.hip), bit for bit against the GPU's own uniform chain:
`render_var` with prev_count = j and spp_offset = j S saved after each pass,
the numpy selection (tests/_adaptive_ref.py) applied to those images, and the
per-unit counters of each uniform pass for the work counters.  Besides the
64x48 frame: packed pixel counts that leave the last wave or workgroup partly
filled, lists of one pixel, of less than a wave and of about one wave, window
radii up to 4, and chunk lengths that are no powers of two.
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


def _chain(mcpt, W, H, S, chunk, passes, spp_offset=0, **fields):
    """[(fb, var) after j + 1 chained uniform render_var calls], computed once per frame and
    left unchanged (a longer chain of the same frame serves the shorter ones); fields: render
    params that change the image (seed), the same in every call"""
    key = (W, H, S, chunk, spp_offset, tuple(sorted(fields.items())))
    have = _chains.setdefault(key, [])
    scene = _scene(mcpt)
    while len(have) < passes:
        j = len(have)
        fb, var = (have[-1][0].copy(), have[-1][1].copy()) if j else (None, None)
        fb, var, _ = scene.render_var(mcpt.RenderParams(width=W, height=H, spp=S, spp_chunk=chunk,
                                                        spp_offset=spp_offset + j * S, prev_count=j, **fields), fb, var)
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


def _pass_counters(mcpt, W, H, S, chunk, passes, tile=8, spp_offset=0, **fields):
    """(passes, H, W, 4) uint64: rays, inner, leaf, tests of every pixel in every uniform pass
    (summed over the pass's chunks), from render_unit_counters; W and H multiples of the tile"""
    key = (W, H, S, chunk, passes, tile, spp_offset, tuple(sorted(fields.items())))
    if key not in _counters:
        assert W % tile == 0 and H % tile == 0
        inv, npix, nch = _unit_order(mcpt, W, H, tile), W * H, (S + chunk - 1) // chunk
        out = np.zeros((passes, H * W, 4), np.uint64)
        for j in range(passes):
            _, uc = _scene(mcpt).render_unit_counters(mcpt.RenderParams(width=W, height=H, spp=S, spp_chunk=chunk,
                                                                        spp_offset=spp_offset + j * S, tile=tile,
                                                                        **fields))
            assert uc.shape == (npix * nch, 4)
            out[j] = uc.reshape(nch, npix, 4).astype(np.uint64).sum(axis=0)[inv]
        _counters[key] = out.reshape(passes, H, W, 4)
    return _counters[key]


def _reference(mcpt, W, H, S, chunk, passes, ap, **chain_kw):
    chain = _chain(mcpt, W, H, S, chunk, passes, **chain_kw)
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
                                                                     "tri_tests"), **counter_kw):
    pc = _pass_counters(mcpt, W, H, S, chunk, passes, **counter_kw)
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


# ---- awkward packed counts, short lists, odd chunk lengths -----------------------------

def _packed_count(mcpt, W, H, tile):
    return len(mcpt.RenderParams(width=W, height=H, tile=tile, packed=True).shard_pixels())


def _list_sizes(chain, passes, ap):
    """pixels listed by every pass after pass 0, from the reference's active sets"""
    active = AR.adaptive_from_chain(chain, max_passes=passes, min_passes=ap.get("min_passes", 1),
                                    threshold=ap["threshold"], lum_floor=ap.get("lum_floor", 0.01),
                                    dilate_r=ap.get("dilate_r", 1))[3]
    return [int(a.sum()) for a in active[1:]]


SMALL_FRAMES = [
    # tile, W, H, packed pixels, render fields
    (1, 37, 29, 1073, {}),
    (4, 36, 28, 1008, {}),
    (5, 37, 29, 1200, {}),
    (8, 24, 8, 192, {}),                        # three waves of one block
    (8, 8, 8, 64, {}),                          # one wave
    (8, 1, 1, 64, dict(spp_offset=48)),         # one real pixel; samples 48..55: the first with radiance (oracle)
]


@pytest.mark.parametrize("case", SMALL_FRAMES, ids=lambda c: f"tile{c[0]}-{c[1]}x{c[2]}")
def test_adaptive_at_awkward_packed_counts_equals_the_uniform_chain(mcpt, case):
    tile, W, H, npk, fields = case
    assert _packed_count(mcpt, W, H, tile) == npk and npk % 256 != 0
    assert npk % 64 != 0 or tile == 8
    frame = dict(W=W, H=H, S=8, chunk=2, passes=4)
    ap = dict(threshold=0.5)
    ref = _reference(mcpt, **frame, ap=ap, **fields)
    sizes = _list_sizes(ref[0], 4, ap)
    print("listed", sizes, "count histogram", np.bincount(ref[3].ravel()).tolist())
    assert len(sizes) == 3 and all(0 < n < npk for n in sizes)      # every later pass runs over a list
    got = _run(mcpt, _scene(mcpt), **frame, ap=ap, tile=tile, **fields)
    _check_images(got, ref, frame["S"])
    if W % tile == 0 and H % tile == 0:
        _check_counters(mcpt, got[3], ref[3], **frame, tile=tile, **fields)


SHORT_LISTS = [
    # threshold, what the reference's lists must contain: (lo, hi) = a pass listing lo..hi pixels
    (0.97, [(1, 1), (2, 63)]),
    (0.95, [(65, 127), (2, 63)]),
    (0.98, [(2, 63)]),
]


@pytest.mark.parametrize("threshold,wanted", SHORT_LISTS, ids=[f"threshold-{t}" for t, _ in SHORT_LISTS])
def test_short_lists_equal_the_uniform_chain(mcpt, threshold, wanted):
    """lists of one pixel, of less than a wave and of one wave and a little: list_kernel's unit
    handout reserves 64 units of which most do not exist"""
    ap = dict(threshold=threshold, dilate_r=0)
    ref = _reference(mcpt, **MAIN, ap=ap)
    sizes = _list_sizes(ref[0], MAIN["passes"], ap)
    print("threshold", threshold, "listed", sizes)
    for lo, hi in wanted:
        assert any(lo <= n <= hi for n in sizes), (lo, hi, sizes)
    got = _run(mcpt, _scene(mcpt), **MAIN, ap=ap)
    _check_images(got, ref, MAIN["S"])
    _check_counters(mcpt, got[3], ref[3], **MAIN)


FORCED = [
    # tile, W, H, list length = packed pixels, render fields
    (8, 8, 8, 64, {}),
    (1, 9, 7, 63, {}),
    (1, 13, 5, 65, {}),
    (8, 1, 1, 64, dict(spp_offset=48)),         # one real pixel
]


@pytest.mark.parametrize("case", FORCED, ids=lambda c: f"tile{c[0]}-{c[1]}x{c[2]}")
def test_force_list_over_lists_of_about_one_wave(mcpt, case):
    """min_passes = max_passes = 3 through the list: the list is the packed frame"""
    tile, W, H, npk, fields = case
    assert _packed_count(mcpt, W, H, tile) == npk
    frame = dict(W=W, H=H, S=8, chunk=2, passes=3)
    chain = _chain(mcpt, W, H, 8, 2, 3, **fields)
    assert chain[2][1][..., :3].max() > 0
    ap = dict(threshold=0.5, min_passes=3, force_list=True)
    fb, var, count, st = _run(mcpt, _scene(mcpt), **frame, ap=ap, tile=tile, **fields)
    assert (count == 3).all()
    _assert_equal(fb, chain[2][0], "framebuffer")
    _assert_equal(var, chain[2][1], "variance")
    assert st["paths"] == 3 * 8 * W * H and st["renders"] == 3
    if W % tile == 0 and H % tile == 0:
        _check_counters(mcpt, st, count, **frame, tile=tile, **fields)


@pytest.mark.parametrize("dilate_r", [2, 4])
def test_wider_dilation_windows(mcpt, dilate_r):
    ap = dict(threshold=0.98, dilate_r=dilate_r)
    ref = _reference(mcpt, **MAIN, ap=ap)
    sizes = _list_sizes(ref[0], MAIN["passes"], ap)
    bare = _list_sizes(ref[0], MAIN["passes"], dict(threshold=0.98, dilate_r=0))
    print("radius", dilate_r, "listed", sizes, "without a window", bare)
    assert sizes and bare and bare[0] < sizes[0] <= bare[0] * (2 * dilate_r + 1) ** 2
    got = _run(mcpt, _scene(mcpt), **MAIN, ap=ap)
    _check_images(got, ref, MAIN["S"])
    _check_counters(mcpt, got[3], ref[3], **MAIN)


def test_a_dilation_window_larger_than_the_frame(mcpt):
    """radius 4 on 6x5: one noisy pixel keeps all 30 active"""
    frame = dict(W=6, H=5, S=8, chunk=2, passes=4)
    ap = dict(threshold=0.5, dilate_r=4)
    ref = _reference(mcpt, **frame, ap=ap)
    assert _list_sizes(ref[0], 4, ap) == [30, 30, 30]
    over = AR.over(ref[0][0][0], ref[0][0][1], 0.5, 0.01)
    assert 0 < int(over.sum()) < 30                                  # the window, not the pixels themselves
    got = _run(mcpt, _scene(mcpt), **frame, ap=ap)
    _check_images(got, ref, frame["S"])
    assert (got[2] == 4).all()


@pytest.mark.parametrize("ap,fields", [(dict(threshold=0.5, lum_floor=0.2), {}),
                                       (dict(threshold=0.5), dict(spp_offset=1000, seed=12345))],
                         ids=["lum-floor-0.2", "offset-1000-seed-12345"])
def test_other_fields_reach_the_selection_and_the_list_kernel(mcpt, ap, fields):
    ref = _reference(mcpt, **MAIN, ap=ap, **fields)
    base = _reference(mcpt, **MAIN, ap=dict(threshold=0.5))
    assert not np.array_equal(ref[3], base[3])                       # the field changes the selection
    hist = np.bincount(ref[3].ravel())
    assert (hist > 0).sum() >= 3, hist.tolist()
    got = _run(mcpt, _scene(mcpt), **MAIN, ap=ap, **fields)
    _check_images(got, ref, MAIN["S"])
    _check_counters(mcpt, got[3], ref[3], **MAIN, **fields)


@pytest.mark.parametrize("kw", [{}, dict(tail_units=500)], ids=["defaults", "mixed-tail-500"])
@pytest.mark.parametrize("S,chunk", [(15, 7), (10, 3)])
def test_chunk_lengths_that_are_no_powers_of_two(mcpt, S, chunk, kw):
    """chunks of 7 7 1 and 3 3 3 1: the merge's d = P_c / n - mean rounds"""
    frame = dict(W=64, H=48, S=S, chunk=chunk, passes=4)
    ap = dict(threshold=0.5)
    ref = _reference(mcpt, **frame, ap=ap)
    hist = np.bincount(ref[3].ravel(), minlength=5)
    assert (hist[1:] > 0).all(), hist.tolist()
    got = _run(mcpt, _scene(mcpt), **frame, ap=ap, **kw)
    _check_images(got, ref, S)
    _check_counters(mcpt, got[3], ref[3], **frame)


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
