"""The wavefront form of the device radiance queries (mcpt_radiance_ex_device,
mcpt_radiance_ex with pipeline = wavefront) on torch tensors, bit for bit against
the megakernel form (Scene.radiance[_device], itself pinned to the CPU oracle by
tests/test_gpu_radiance.py) and, where named, against a wavefront render.

Every comparison is np.array_equal on the float bits; every output tensor carries
64 guard elements behind it (tests/_radiance_q.py).  Counters: a wavefront query
counts rays, paths and shades as the counting megakernel query does; its four
visit counters equal that query's on a counting call and read 0 on a lean one.

A render's primary rays: a query traces every sample of a ray along the one ray
it was given, while a render jitters each sample's primary ray, so one call of
spp = 5 cannot reproduce a 5-spp render.  The case is therefore run both ways:
one call of spp = 5, spp_chunk = 2 along the frame's sample-0 rays against the
megakernel query's call, and the render itself from five one-sample calls along
each sample's own rays, summed as the kernels sum (as tests/test_gpu_radiance.py
pins the megakernel form to its render).
"""
import numpy as np
import pytest

import _aov_ref as A
from _radiance_q import (COUNTERS, CONFIGS, GUARD, SENT, VISITS, Ctx, add_counters, bits, check_counters, combine,
                         counted, f32, query, same)

pytestmark = pytest.mark.gpu

WF = {}                                   # the wavefront form with every wavefront field automatic


@pytest.fixture(scope="module")
def ctx(mcpt, oracle_mod):
    return Ctx(mcpt, oracle_mod)


# ---- 1. a render's primary rays ---------------------------------------------------

@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("key", ["scene01", "scene01-global", "scene03"])
def test_primary_rays_of_a_render(ctx, mcpt, key, lean):
    W, H, spp, chunk = 37, 29, 5, 2
    scene, eye, look = ctx.scene(key), CONFIGS[key][2], CONFIGS[key][3]
    orc = ctx.oracle
    ids = np.arange(W * H, dtype=np.uint32)
    rays = [A.primary_rays(orc, W, H, 1, spp_offset=s, eye=eye, direction=look) for s in range(spp)]
    # one call of spp samples along the frame's sample-0 rays: the megakernel query's bits and counters
    o0, d0 = rays[0]
    ref, rs = ctx.reference(("primary", key), key, o0, d0, ids=ids, spp=spp, spp_chunk=chunk)
    got, st = counted(scene, o0, d0, ids=ids, wf=WF, spp=spp, spp_chunk=chunk, lean=lean)
    assert same(got, ref), (key, lean, int((bits(got) != bits(ref)).sum()))
    check_counters(st, rs, lean, key)
    assert st["paths"] == W * H * spp and (got > 0).any()
    # the wavefront render of the frame, from each sample's own primary rays
    p = mcpt.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, eye=eye, direction=look, pipeline="wavefront",
                          lean=bool(lean))
    img, rst = scene.render(p)
    assert rst["variant"] in (4, 5)
    scene.trace_stats()
    samples = [query(scene, o, d, ids=ids, wf=WF, spp=1, spp_offset=s, lean=lean) for s, (o, d) in enumerate(rays)]
    total = scene.trace_stats()
    routes = scene.query_route_rays()
    assert same(combine(samples, chunk).reshape(H, W, 3), img), (key, lean)
    for k in ("rays", "paths", "shades") + (() if lean else VISITS):
        assert total[k] == rst[k], (key, lean, k, total[k], rst[k])
    # the host entry names the layout
    n = 512
    _, hst = scene.radiance_ex(o0.reshape(-1, 3)[:n], d0.reshape(-1, 3)[:n], pipeline="wavefront", lean=lean)
    assert hst["variant"] == (4 if scene.info()["node_boxes"] == 0 else 5)
    if key == "scene01" and lean:
        assert routes[0] > 0 and routes[0] == rst["direct_rays"], (routes, rst["direct_rays"])
    if not lean:
        assert routes[0] == 0 and routes[2] == 0 and routes[3] == 0       # counting queries walk every ray


# ---- 2. origins that are not the eye ------------------------------------------------

@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_origins_that_are_not_the_eye(ctx, key, depth, lean):
    scene = ctx.scene(key)
    if depth == 0:
        (o, d), params = ctx.rays(key, 20_000), dict(spp=1, max_depth=0)
    else:
        (o, d), params = ctx.unit_rays(key, 20_000), dict(spp=3, spp_chunk=2, max_depth=2)
    assert o.shape[0] == 20_000 and len(np.unique(o, axis=0)) > 1000
    ref, rs = ctx.reference(("origins", key, depth), key, o, d, **params)
    got, st = counted(scene, o, d, wf=WF, lean=lean, **params)
    assert same(got, ref), (key, depth, lean, int((bits(got) != bits(ref)).sum()))
    check_counters(st, rs, lean, (key, depth))
    assert (ref > 0).any() and st["paths"] == params["spp"] * 20_000
    assert (st["shades"] > 0) == (depth > 0)


# ---- 3. shapes ------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_small_and_odd_batches_equal_slices_of_the_megakernel_query(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.unit_rays(key, 5000)
    big, _ = ctx.reference(("shapes", key), key, o[:4097], d[:4097], spp=3, spp_chunk=2)
    for n in (1, 63, 64, 65, 1025, 4097):
        for lean in (1, 0):
            got, st = counted(scene, o[:n], d[:n], wf=WF, spp=3, spp_chunk=2, lean=lean)
            assert same(got, big[:n]), (key, n, lean)
            assert st["paths"] == 3 * n


SCHEDULES = [dict(wf_batch=2), dict(wf_batch=64), dict(wf_batch=1000), dict(wf_streams=1), dict(wf_streams=3),
             dict(wf_streams=4), dict(wf_refill=1), dict(wf_refill=64), dict(wf_sort=1),
             dict(wf_batch=1000, wf_streams=3, wf_sort=1)]


@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_scheduling_never_changes_a_result(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.unit_rays(key, 5000)
    o, d = o[:1025], d[:1025]
    ref, rs = ctx.reference(("sched", key), key, o, d, spp=7, spp_chunk=3)
    extra = [dict(wf_group_shift=6), dict(wf_group_shift=0), dict(wf_group_shift=6, wf_batch=1000)] if "global" in key else []
    for kw in SCHEDULES + extra:
        for lean in (1, 0):
            got, st = counted(scene, o, d, wf=kw, spp=7, spp_chunk=3, lean=lean)
            assert same(got, ref), (key, kw, lean, int((bits(got) != bits(ref)).sum()))
            check_counters(st, rs, lean, (key, kw))


# ---- 4. parameters --------------------------------------------------------------------

@pytest.mark.parametrize("params", [dict(max_depth=0), dict(max_depth=1), dict(max_depth=7), dict(fresnel_kd=0),
                                    dict(fresnel_kd=1), dict(seed=0x1234567890ABCDEF)])
def test_parameters_reach_the_kernels(ctx, params):
    scene = ctx.scene("scene01")
    o, d = ctx.unit_rays("scene01", 2000)
    ref, rs = counted(scene, o, d, spp=2, **params)
    for lean in (1, 0):
        got, st = counted(scene, o, d, wf=WF, spp=2, lean=lean, **params)
        assert same(got, ref), (params, lean)
        check_counters(st, rs, lean, params)
    base = ctx.reference(("params", "base"), "scene01", o, d, spp=2)[0]
    if params not in (dict(max_depth=7), dict(fresnel_kd=1)):          # (the defaults)
        assert not same(ref, base), params


@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_several_samples_are_the_chunk_sum_of_single_wavefront_samples(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.unit_rays(key, 2000)
    spp, chunk, off = 7, 3, 2
    for lean in (1, 0):
        samples, total = [], {}
        for s in range(spp):
            r, st = counted(scene, o, d, wf=WF, spp=1, spp_offset=off + s, lean=lean)
            samples.append(r)
            add_counters(total, st)
        got, st = counted(scene, o, d, wf=WF, spp=spp, spp_chunk=chunk, spp_offset=off, lean=lean)
        assert same(got, combine(samples, chunk)), (key, lean)
        for k in COUNTERS:
            assert st[k] == total[k], (key, lean, k, st[k], total[k])
        assert st["paths"] == spp * o.shape[0] and st["shades"] > 0
    assert same(got, ctx.reference(("chunks", key), key, o, d, spp=spp, spp_chunk=chunk, spp_offset=off)[0])


def test_running_mean_over_two_chained_calls(ctx):
    scene = ctx.scene("scene01")
    o, d = ctx.unit_rays("scene01", 2000)
    a = query(scene, o, d, spp=4, spp_offset=0)
    b = query(scene, o, d, spp=4, spp_offset=4)
    want = ((a * f32(1) + b) / f32(2)).astype(f32)
    first = query(scene, o, d, wf=WF, spp=4, spp_offset=0, prev_count=0, prev=np.full_like(a, 77.0))   # old content not read
    assert same(first, a)
    assert same(query(scene, o, d, wf=WF, spp=4, spp_offset=4, prev_count=1, prev=first), want)
    # the first call on the megakernel, the second on the wavefront
    assert same(query(scene, o, d, wf=dict(wf_streams=1), spp=4, spp_offset=4, prev_count=1, prev=a), want)
    assert not same(a, b)


def test_stream_ids_default_to_the_index_and_batches_split_and_shuffle(ctx):
    scene = ctx.scene("scene01")
    o, d = ctx.unit_rays("scene01", 2000)
    n, h = o.shape[0], o.shape[0] // 2
    whole = ctx.reference(("ids", "whole"), "scene01", o, d, spp=2)[0]
    assert same(query(scene, o, d, wf=WF, spp=2), whole)
    assert same(query(scene, o, d, ids=np.arange(n), wf=WF, spp=2), whole)
    lo = query(scene, o[:h], d[:h], wf=WF, spp=2)
    hi = query(scene, o[h:], d[h:], ids=np.arange(h, n), wf=WF, spp=2)
    assert same(np.concatenate([lo, hi]), whole)
    assert not same(query(scene, o[h:], d[h:], wf=WF, spp=2), whole[h:])      # (the ids matter)
    perm = np.random.default_rng(5).permutation(n)
    assert same(query(scene, o[perm], d[perm], ids=np.arange(n)[perm], wf=WF, spp=2), whole[perm])


# ---- 5. plumbing ----------------------------------------------------------------------

def test_reserve_then_no_allocation(mcpt, ctx):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))      # a scene that has run nothing
    o, d = ctx.unit_rays("scene01", 5000)
    n = o.shape[0]
    want = query(ctx.scene("scene01"), o, d, spp=6, spp_chunk=2)
    want_small = query(ctx.scene("scene01"), o[:3000], d[:3000], spp=4, spp_chunk=2)
    p = mcpt.RenderParams(width=64, height=48, spp=4)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    out = torch.full((4 * n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.reserve_radiance_ex(n, pipeline="wavefront", spp=6, spp_chunk=2, lean=1)
    free0 = scene.plan(p)["device_free_bytes"]
    for _ in range(2):
        out.fill_(SENT)
        scene.radiance_ex_device(n, d_o.data_ptr(), d_d.data_ptr(), out.data_ptr(), pipeline="wavefront", spp=6,
                                 spp_chunk=2, lean=1)
        torch.cuda.synchronize()
        assert scene.plan(p)["device_free_bytes"] == free0
        h = out.cpu().numpy()
        assert same(h[:4 * n].reshape(n, 4)[:, :3], want) and (h[4 * n:] == f32(SENT)).all()
    # fewer rays and fewer chunks than reserved
    out.fill_(SENT)
    scene.radiance_ex_device(3000, d_o.data_ptr(), d_d.data_ptr(), out.data_ptr(), pipeline="wavefront", spp=4,
                             spp_chunk=2, lean=1)
    torch.cuda.synchronize()
    assert scene.plan(p)["device_free_bytes"] == free0
    h = out.cpu().numpy()
    assert same(h[:12000].reshape(3000, 4)[:, :3], want_small) and (h[12000:] == f32(SENT)).all()
    assert scene.trace_stats()["paths"] == 2 * 6 * n + 4 * 3000
    # n = 0 is a no-op on either pipeline
    for pipeline in ("wavefront", "megakernel"):
        scene.radiance_ex_device(0, 0, 0, 0, pipeline=pipeline)
        scene.reserve_radiance_ex(0, pipeline=pipeline)
        e, st = scene.radiance_ex(np.zeros((0, 3), f32), np.zeros((0, 3), f32), pipeline=pipeline)
        assert e.shape == (0, 3) and st["rays"] == 0
    assert scene.trace_stats()["rays"] == 0 and scene.plan(p)["device_free_bytes"] == free0


def test_query_on_a_torch_stream(ctx):
    import torch
    scene = ctx.scene("scene01")
    o, d = ctx.unit_rays("scene01", 2000)
    ref = ctx.reference(("stream",), "scene01", o, d, spp=2)[0]
    st = torch.cuda.Stream()
    assert same(query(scene, o, d, wf=WF, spp=2, stream=st), ref)
    assert same(query(scene, o, d, wf=dict(wf_streams=3, wf_batch=1000), spp=2, stream=st), ref)


@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_the_host_entry_equals_the_device_entry(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.unit_rays(key, 2000)
    ids = (np.arange(o.shape[0], dtype=np.uint32) * 7 + 3).astype(np.uint32)
    for lean in (1, 0):
        ref, rs = counted(scene, o, d, ids=ids, wf=WF, spp=3, spp_chunk=2, lean=lean)
        got, st = scene.radiance_ex(o, d, stream_ids=ids, pipeline="wavefront", spp=3, spp_chunk=2, lean=lean)
        assert got.shape == (o.shape[0], 3) and same(got, ref)
        for k in COUNTERS:
            assert st[k] == rs[k], (k, st[k], rs[k])
        assert st["variant"] == (5 if "global" in key else 4)
        z = scene.trace_stats()                           # the host entry leaves the device entries' block alone
        assert all(z[k] == 0 for k in COUNTERS) and scene.query_route_rays() == (0, 0, 0, 0)
    nxt, _ = scene.radiance_ex(o, d, stream_ids=ids, pipeline="wavefront", spp=3, spp_chunk=2, spp_offset=3, prev_count=1,
                               prev=got)
    assert same(nxt, query(scene, o, d, ids=ids, spp=3, spp_chunk=2, spp_offset=3, prev_count=1, prev=ref))


def test_overlapping_buffers_are_refused_and_left_alone(mcpt, ctx):
    import torch
    scene = ctx.scene("scene01")
    n = 1024
    o, d = ctx.unit_rays("scene01", n)
    buf = torch.full((16 * n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    buf[:3 * n] = torch.from_numpy(o.ravel()).cuda()
    buf[3 * n:6 * n] = torch.from_numpy(d.ravel()).cuda()
    buf[6 * n:7 * n] = torch.from_numpy(np.arange(n, dtype=np.int32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    before = buf.cpu().numpy().copy()
    base = buf.data_ptr()
    O, D, S, FREE = base, base + 12 * n, base + 24 * n, base + 28 * n
    scene.trace_stats()
    for kw in (dict(out_ptr=O), dict(out_ptr=O + 12 * n - 4), dict(out_ptr=D + 12 * n - 4),
               dict(out_ptr=FREE, stream_ids_ptr=FREE + 16 * n - 4), dict(out_ptr=S + 4 * n - 4, stream_ids_ptr=S),
               dict(out_ptr=O - 16 * n + 4)):
        with pytest.raises(mcpt.McptError) as e:
            scene.radiance_ex_device(n, O, D, pipeline="wavefront", **kw)
        assert e.value.code == -1 and "overlap" in str(e.value), kw
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
    assert scene.trace_stats()["rays"] == 0
    # adjacent, not overlapping: accepted
    scene.radiance_ex_device(n, O, D, FREE, S, pipeline="wavefront", spp=2)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert same(got[7 * n:11 * n].reshape(n, 4)[:, :3], query(scene, o, d, spp=2))
    assert np.array_equal(got[:7 * n].view(np.uint32), before[:7 * n].view(np.uint32))
    assert (got[11 * n:] == f32(SENT)).all()


@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_the_megakernel_pipeline_through_the_ex_entries_is_the_old_entries(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.unit_rays(key, 2000)
    names = COUNTERS + ("stack_spills", "renders", "variant", "devices")
    for lean in (0, 1):
        ref, rs = counted(scene, o, d, spp=3, spp_chunk=2, lean=lean)
        got, st = counted(scene, o, d, ex=True, spp=3, spp_chunk=2, lean=lean)
        assert same(got, ref)
        for k in names:
            assert st[k] == rs[k], (k, st[k], rs[k])
        assert scene.query_route_rays() == (0, 0, 0, 0)
        h0, hs0 = scene.radiance(o, d, spp=3, spp_chunk=2, lean=lean)
        h1, hs1 = scene.radiance_ex(o, d, spp=3, spp_chunk=2, lean=lean)
        assert same(h1, h0) and same(h0, ref)
        for k in names:
            assert hs1[k] == hs0[k], (k, hs1[k], hs0[k])


def test_a_two_replica_scene_answers_on_its_first_device(mcpt, ctx):
    o, d = ctx.unit_rays("scene01", 2000)
    tr = mcpt.Tracer()
    try:
        tr.initialize([0, 0])
        multi = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
        assert multi.info()["n_devices"] == 2
        got, st = counted(multi, o, d, wf=WF, spp=3, spp_chunk=2, lean=1)
        routes = multi.query_route_rays()
    finally:
        tr.initialize([0])
    single = ctx.scene("scene01")
    ref, rs = counted(single, o, d, wf=WF, spp=3, spp_chunk=2, lean=1)
    assert same(got, ref) and same(ref, query(single, o, d, spp=3, spp_chunk=2))
    for k in COUNTERS:
        assert st[k] == rs[k], (k, st[k], rs[k])
    assert routes == single.query_route_rays()


# ---- 6. nothing else moves ---------------------------------------------------------------

@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_queries_leave_the_render_state_alone(mcpt, ctx, pipeline):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    p = mcpt.RenderParams(width=64, height=48, spp=4, spp_chunk=2, pipeline=pipeline, lean=True)
    img0, st0 = scene.render(p)
    classes0 = scene.primary_tile_classes()
    routes = ("direct_rays", "extend_rays", "clipped_rays", "primary_shaded", "sphere_skips")
    if pipeline == "wavefront":
        assert st0["direct_rays"] > 0 and st0["primary_shaded"] > 0 and classes0["listed"] > 0
    o, d = ctx.unit_rays("scene01", 2000)
    ref = ctx.reference(("state",), "scene01", o, d, spp=2)[0]
    for lean in (1, 0):
        assert same(query(scene, o, d, wf=WF, spp=2, lean=lean), ref)
    got, _ = scene.radiance_ex(o, d, pipeline="wavefront", spp=2, lean=1)
    assert same(got, ref)
    # the record the render left is as it was, and a new read finds nothing rendered
    lib = mcpt.lib()
    for k in routes:
        assert int(getattr(lib, "mcpt_scene_" + k)(scene.handle)) == st0[k], k
    assert scene.primary_tile_classes() == classes0
    z = scene.stats()
    for k in COUNTERS + ("stack_spills", "renders") + routes:
        assert z[k] == 0, (k, z[k])
    assert scene.primary_tile_classes() == classes0
    # the same render after the queries: the same bits and the same record
    img1, st1 = scene.render(p)
    assert same(img0, img1)
    for k in COUNTERS + ("renders", "variant") + routes:
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    assert scene.primary_tile_classes() == classes0
    assert scene.trace_stats()["paths"] == 2 * 2 * o.shape[0]            # and the render left the queries' alone


def test_the_host_entry_reports_its_own_call_after_lean_device_queries(ctx):
    """the route counters of the wavefront's kernels lie behind the eight Counters: a query that
    counted into an eight-word block would spill them into the neighbouring block"""
    scene = ctx.scene("scene01")
    o, d = ctx.unit_rays("scene01", 5000)
    _, one = counted(scene, o[:700], d[:700], spp=1)                             # what the host call is to report
    for _ in range(3):
        query(scene, o, d, wf=WF, spp=2, lean=1)
    got, st = scene.radiance_ex(o[:700], d[:700], pipeline="wavefront", spp=1, lean=1)
    for k in ("rays", "paths", "shades"):
        assert st[k] == one[k], (k, st[k], one[k])
    for k in VISITS + ("stack_spills",):
        assert st[k] == 0, (k, st[k])
    got_mk, st_mk = scene.radiance(o[:700], d[:700], spp=1)                      # the megakernel host entry as well
    for k in COUNTERS:
        assert st_mk[k] == one[k], (k, st_mk[k], one[k])
    assert same(got, got_mk)
    dev = scene.trace_stats()
    assert dev["paths"] == 3 * 2 * 5000 and scene.query_route_rays()[0] > 0


def test_trace_stats_after_a_mixed_sequence_is_the_sum(ctx):
    scene = ctx.scene("scene01")
    o, d = ctx.unit_rays("scene01", 2000)
    n = o.shape[0]
    import torch
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def hits():
        scene.trace_device(n, d_o.data_ptr(), d_d.data_ptr(), tri.data_ptr())
        torch.cuda.synchronize()

    parts = []
    scene.trace_stats()
    hits()
    parts.append(scene.trace_stats())
    parts.append(counted(scene, o, d, spp=2)[1])
    parts.append(counted(scene, o, d, wf=WF, spp=2, lean=0)[1])
    count_routes = scene.query_route_rays()
    parts.append(counted(scene, o, d, wf=WF, spp=3, lean=1)[1])
    lean_routes = scene.query_route_rays()
    scene.trace_stats()
    hits()
    query(scene, o, d, spp=2)
    query(scene, o, d, wf=WF, spp=2, lean=0)
    query(scene, o, d, wf=WF, spp=3, lean=1)
    total = scene.trace_stats()
    for k in COUNTERS + ("stack_spills",):
        assert total[k] == sum(p[k] for p in parts), (k, total[k], [p[k] for p in parts])
    assert total["rays"] > parts[0]["rays"] > 0
    assert scene.query_route_rays() == tuple(a + b for a, b in zip(count_routes, lean_routes))
    assert lean_routes[0] > 0 and count_routes[0] == 0 and count_routes[1] > 0
