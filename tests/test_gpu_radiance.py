"""Device radiance queries (mcpt_radiance_device, mcpt_radiance) on torch
tensors, bit for bit against references that are pinned themselves: the CPU
oracle's render and the megakernel's (a render's primary rays, queried sample by
sample and summed as the kernels sum, give the render's image and counters),
the oracle's ordered walk (depth 0: the emission at the closest hit) and the
query itself (several samples = the chunk sum of single samples, the running
mean, stream ids, batch shapes, scheduling, plumbing).

Every comparison is np.array_equal on the float bits.  Every output tensor
carries 64 guard elements behind it, checked after every query.
"""
import numpy as np
import pytest

import _aov_ref as A
from _raysets import ray_sets
from _var_ref import chunk_lengths

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64
SENT = -123.5
SEED = 0x4D435054
VISITS = ("inner_visits", "leaf_visits", "leaf_refs", "tri_tests")
COUNTERS = ("rays", "paths", "shades") + VISITS
# key -> (scene, layout, eye, direction).  scene03 is a closed room: its default camera, outside, renders
# black in the oracle too, so its case looks at the light from inside
CONFIGS = {
    "scene01": ("scene01", "auto", (0.0, 5.0, 17.0), (0.0, 0.0, -1.0)),
    "scene01-global": ("scene01", "global", (0.0, 5.0, 17.0), (0.0, 0.0, -1.0)),
    "scene03": ("scene03", "auto", (0.0, 5.0, 4.0), (0.0, 0.5, -1.0)),
}


class Ctx:
    """scenes, oracle scenes and ray sets, each made once"""

    def __init__(self, mcpt, oracle_mod):
        self.mcpt, self.oracle = mcpt, oracle_mod
        self._scene, self._oscene, self._rays = {}, {}, {}

    def scene(self, key):
        if key not in self._scene:
            name, layout = CONFIGS[key][:2]
            self._scene[key] = self.mcpt.Scene(self.mcpt.ObjModel(self.mcpt.scene_path(name)), layout=layout)
        return self._scene[key]

    def oscene(self, key):
        name = CONFIGS[key][0]
        if name not in self._oscene:
            self._oscene[name] = self.oracle.Scene(self.mcpt.scene_path(name))
        return self._oscene[name]

    def rays(self, key, n):
        """the first n of ray_sets(oracle scene, 20 000, seed 23) spread over all families"""
        name = CONFIGS[key][0]
        if name not in self._rays:
            self._rays[name] = ray_sets(self.oscene(key), 20_000, seed=23)
        o, d = self._rays[name]
        sel = np.arange(n) * (o.shape[0] // n)
        return np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])


@pytest.fixture(scope="module")
def ctx(mcpt, oracle_mod):
    return Ctx(mcpt, oracle_mod)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def query(scene, o, d, ids=None, stream=None, prev=None, **params):
    """Scene.radiance_device on fresh torch tensors -> (n, 3) float32; the fourth component is
    0 and the guard behind the output untouched.  prev: the output's old content (n, 3)"""
    import torch
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    n = o.shape[0]
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32)).cuda() if ids is not None else None
    out = torch.full((4 * n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    if prev is not None:
        old = np.zeros((n, 4), np.float32)
        old[:, :3] = prev
        out[:4 * n] = torch.from_numpy(old.ravel()).cuda()
    torch.cuda.synchronize()
    scene.radiance_device(n, d_o.data_ptr(), d_d.data_ptr(), out.data_ptr(), d_s.data_ptr() if d_s is not None else 0,
                          stream.cuda_stream if stream is not None else 0, **params)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[4 * n:] == f32(SENT)).all(), "guard behind the radiance overwritten"
    h = h[:4 * n].reshape(n, 4)
    assert (h[:, 3] == 0).all() and not np.signbit(h[:, 3]).any()
    return np.ascontiguousarray(h[:, :3])


def combine(samples, chunk):
    """per-sample results (spp, ...) -> the kernels' mean: in order from 0 inside chunks of
    `chunk`, the chunk sums in order from 0, divided by (float)spp"""
    spp = len(samples)
    total, k = np.zeros_like(samples[0]), 0
    for n in chunk_lengths(spp, chunk if chunk else spp):
        P = np.zeros_like(samples[0])
        for _ in range(n):
            P = (P + samples[k]).astype(f32)
            k += 1
        total = (total + P).astype(f32)
    return (total / f32(spp)).astype(f32)


def add_counters(total, st):
    for k in COUNTERS:
        total[k] = total.get(k, 0) + st[k]
    return total


# ---- 1. a render's primary rays give the render's image ------------------------

@pytest.mark.parametrize("key,max_depth,fresnel_kd,seed", [
    ("scene01", 7, 1, SEED), ("scene01-global", 7, 1, SEED), ("scene03", 7, 1, SEED), ("scene01", 0, 1, SEED),
    ("scene01", 1, 1, SEED), ("scene01", 7, 0, SEED), ("scene01", 7, 1, 0x1234567890ABCDEF)])
def test_primary_rays_of_a_render_give_its_image_and_counters(ctx, mcpt, key, max_depth, fresnel_kd, seed):
    W, H, spp, chunk = 37, 29, 5, 2
    scene, eye, look = ctx.scene(key), CONFIGS[key][2], CONFIGS[key][3]
    boxes = int(scene.info()["node_boxes"])
    assert boxes == {"scene01": 0, "scene01-global": 1, "scene03": 1}[key]     # (scene03 does not fit in LDS)
    orc = ctx.oracle
    ref, rc = ctx.oscene(key).render(orc.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, max_depth=max_depth,
                                                       eye=eye, direction=look, seed=seed, fresnel_kd=fresnel_kd,
                                                       traversal=orc.KD_ORDERED, threads=8, node_boxes=boxes))
    img, st = scene.render(mcpt.RenderParams(width=W, height=H, spp=spp, spp_chunk=chunk, max_depth=max_depth, eye=eye,
                                             direction=look, seed=seed, fresnel_kd=bool(fresnel_kd), pipeline="megakernel"))
    assert same(img, ref)
    scene.trace_stats()                                   # a fresh record
    samples, total = [], {}
    for s in range(spp):
        o, d = A.primary_rays(orc, W, H, 1, spp_offset=s, seed=seed, eye=eye, direction=look)
        samples.append(query(scene, o, d, spp=1, spp_offset=s, max_depth=max_depth, fresnel_kd=fresnel_kd, seed=seed))
        add_counters(total, scene.trace_stats())
    got = combine(samples, chunk).reshape(H, W, 3)
    assert same(got, ref), (key, int((_bits(got) != _bits(ref)).sum()))
    assert same(got, img)
    for k in COUNTERS:
        assert total[k] == rc[k] == st[k], (k, total[k], rc[k], st[k])
    assert total["paths"] == W * H * spp and (got > 0).any()


# ---- 2. mixed origins in one batch, stream ids given ----------------------------

CAMERAS = [dict(eye=(0.0, 5.0, 17.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=60.0),
           dict(eye=(1.0, 4.0, 3.0), direction=(-0.3, -0.1, -1.0), up=(0.0, 1.0, 0.0), fov=75.0),
           dict(eye=(0.5, 9.0, 1.0), direction=(0.0, -1.0, 0.1), up=(0.0, 0.0, -1.0), fov=50.0)]


@pytest.mark.parametrize("s", [0, 3])
def test_three_cameras_shuffled_into_one_batch_with_stream_ids(ctx, s):
    W, H = 24, 16
    orc, scene = ctx.oracle, ctx.scene("scene01")
    O, D, refs = [], [], []
    for cam in CAMERAS:
        o, d = A.primary_rays(orc, W, H, 1, spp_offset=s, fov=cam["fov"], eye=cam["eye"], direction=cam["direction"],
                              up=cam["up"])
        O.append(o.reshape(-1, 3))
        D.append(d.reshape(-1, 3))
        ref, _ = ctx.oscene("scene01").render(orc.RenderParams(width=W, height=H, spp=1, spp_offset=s, traversal=orc.KD_ORDERED,
                                                               threads=8, **cam))
        refs.append(ref.reshape(-1, 3))
    npx = W * H
    O, D = np.concatenate(O), np.concatenate(D)
    ids = np.tile(np.arange(npx, dtype=np.uint32), 3)
    perm = np.random.default_rng(5).permutation(3 * npx)
    got = query(scene, O[perm], D[perm], ids=ids[perm], spp=1, spp_offset=s)
    back = np.zeros_like(got)
    back[perm] = got
    for c in range(3):
        assert same(back[c * npx:(c + 1) * npx], refs[c]), (s, c)
        assert (refs[c] > 0).any()
    assert not same(refs[0], refs[1]) and not same(refs[0], refs[2])


# ---- 3. depth 0 on adversarial rays ----------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene03"])
def test_depth_zero_is_the_emission_at_the_closest_hit(ctx, key):
    scene, osc = ctx.scene(key), ctx.oscene(key)
    o, d = ctx.rays(key, 20_000)
    n = o.shape[0]
    scene.trace_stats()
    got = query(scene, o, d, spp=1, max_depth=0)
    st = scene.trace_stats()
    tri, geom, _, _ = osc.intersect(o, d, ctx.oracle.KD_ORDERED, threads=8)
    hit = tri >= 0
    ka = osc.geoms()[np.where(hit, geom, 0)][:, 0:3].astype(f32)
    want = np.where(hit[:, None], f32(1) * (ka * f32(10.0)), f32(0)).astype(f32)
    assert same(got, want)
    assert 0.3 < hit.mean() < 1.0 and (want > 0).any()
    _, _, rs = scene.intersect(o, d)
    assert st["rays"] == n == st["paths"] and st["shades"] == 0
    for k in VISITS:
        assert st[k] == rs[k], (k, st[k], rs[k])


# ---- 4. several samples are the chunk sum of single samples ----------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_several_samples_are_the_chunk_sum_of_single_samples(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.rays(key, 2000)
    spp, chunk, off = 7, 3, 2
    scene.trace_stats()
    samples, total = [], {}
    for s in range(spp):
        samples.append(query(scene, o, d, spp=1, spp_offset=off + s))
        add_counters(total, scene.trace_stats())
    got = query(scene, o, d, spp=spp, spp_chunk=chunk, spp_offset=off)
    st = scene.trace_stats()
    assert same(got, combine(samples, chunk))
    for k in COUNTERS:
        assert st[k] == total[k], (k, st[k], total[k])
    assert st["paths"] == spp * o.shape[0] and st["shades"] > 0


# ---- 5. running mean --------------------------------------------------------------

def test_running_mean_over_two_chained_calls(ctx):
    scene = ctx.scene("scene01")
    o, d = ctx.rays("scene01", 2000)
    a = query(scene, o, d, spp=4, spp_offset=0)
    b = query(scene, o, d, spp=4, spp_offset=4)
    first = query(scene, o, d, spp=4, spp_offset=0, prev_count=0, prev=np.full_like(a, 77.0))   # old content not read
    assert same(first, a)
    chained = query(scene, o, d, spp=4, spp_offset=4, prev_count=1, prev=first)
    want = ((a * f32(1) + b) / f32(2)).astype(f32)
    assert same(chained, want)
    assert not same(a, b)


# ---- 6. stream ids, defaults and splitting a batch -------------------------------

def test_stream_ids_default_to_the_index_and_split_batches_agree(ctx):
    scene = ctx.scene("scene01")
    o, d = ctx.rays("scene01", 2000)
    n, h = o.shape[0], o.shape[0] // 2
    whole = query(scene, o, d, spp=2)
    assert same(query(scene, o, d, ids=np.arange(n), spp=2), whole)
    lo = query(scene, o[:h], d[:h], spp=2)
    hi = query(scene, o[h:], d[h:], ids=np.arange(h, n), spp=2)
    assert same(np.concatenate([lo, hi]), whole)
    # (and the ids matter: the second half on the first half's streams differs)
    assert not same(query(scene, o[h:], d[h:], spp=2), whole[h:])


# ---- 7. small and odd batches -----------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_small_and_odd_batches_equal_slices_of_a_larger_query(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.rays(key, 2000)
    big = query(scene, o, d, spp=3, spp_chunk=2)
    for n in (1, 63, 64, 65, 1025):
        scene.trace_stats()
        got = query(scene, o[:n], d[:n], spp=3, spp_chunk=2)
        assert same(got, big[:n]), (key, n)
        assert scene.trace_stats()["paths"] == 3 * n


# ---- 8. scheduling ------------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_scheduling_never_changes_a_result(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.rays(key, 5000)
    scene.trace_stats()
    ref = query(scene, o, d, spp=3)
    rs = scene.trace_stats()
    assert rs["paths"] == 3 * o.shape[0]
    for kw in (dict(workgroups=1), dict(workgroups=3), dict(ready_thresh=1), dict(ready_thresh=64),
               dict(spp_chunk=3), dict(workgroups=2, ready_thresh=7)):
        got = query(scene, o, d, spp=3, **kw)
        st = scene.trace_stats()
        assert same(got, ref), (key, kw)
        for k in COUNTERS:
            assert st[k] == rs[k], (key, kw, k)
    got = query(scene, o, d, spp=3, lean=1)
    st = scene.trace_stats()
    assert same(got, ref)
    assert st["rays"] == rs["rays"]                       # the lean kernel counts rays only
    for k in COUNTERS[1:] + ("stack_spills",):
        assert st[k] == 0, (k, st[k])


# ---- 9. plumbing --------------------------------------------------------------------

def test_reserve_then_no_allocation(mcpt, ctx):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))      # a scene that has run no query
    o, d = ctx.rays("scene01", 5000)
    n = o.shape[0]
    want = query(ctx.scene("scene01"), o, d, spp=6, spp_chunk=2)
    want_small = query(ctx.scene("scene01"), o[:3000], d[:3000], spp=4, spp_chunk=2)
    p = mcpt.RenderParams(width=64, height=48, spp=4)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    out = torch.full((4 * n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.reserve_radiance(n, spp=6, spp_chunk=2)
    free0 = scene.plan(p)["device_free_bytes"]
    for _ in range(2):
        out.fill_(SENT)
        scene.radiance_device(n, d_o.data_ptr(), d_d.data_ptr(), out.data_ptr(), spp=6, spp_chunk=2)
        torch.cuda.synchronize()
        assert scene.plan(p)["device_free_bytes"] == free0
        h = out.cpu().numpy()
        assert same(h[:4 * n].reshape(n, 4)[:, :3], want) and (h[4 * n:] == f32(SENT)).all()
    # fewer rays and fewer chunks than reserved
    out.fill_(SENT)
    scene.radiance_device(3000, d_o.data_ptr(), d_d.data_ptr(), out.data_ptr(), spp=4, spp_chunk=2)
    torch.cuda.synchronize()
    assert scene.plan(p)["device_free_bytes"] == free0
    h = out.cpu().numpy()
    assert same(h[:12000].reshape(3000, 4)[:, :3], want_small) and (h[12000:] == f32(SENT)).all()
    assert scene.trace_stats()["paths"] == 2 * 6 * n + 4 * 3000
    # n = 0 is a no-op
    scene.radiance_device(0, 0, 0, 0)
    assert scene.trace_stats()["rays"] == 0


def test_query_on_a_torch_stream(ctx):
    import torch
    scene = ctx.scene("scene01")
    o, d = ctx.rays("scene01", 2000)
    ref = query(scene, o, d, spp=2)
    assert same(query(scene, o, d, spp=2, stream=torch.cuda.Stream()), ref)


def test_the_host_entry_equals_the_device_entry(ctx):
    scene = ctx.scene("scene01")
    o, d = ctx.rays("scene01", 2000)
    ids = (np.arange(o.shape[0], dtype=np.uint32) * 7 + 3).astype(np.uint32)
    scene.trace_stats()
    ref = query(scene, o, d, ids=ids, spp=3, spp_chunk=2)
    rs = scene.trace_stats()
    got, st = scene.radiance(o, d, stream_ids=ids, spp=3, spp_chunk=2)
    assert got.shape == (o.shape[0], 3) and same(got, ref)
    for k in COUNTERS:
        assert st[k] == rs[k], (k, st[k], rs[k])
    z = scene.trace_stats()                               # the host entry leaves the device entries' block alone
    assert all(z[k] == 0 for k in COUNTERS)
    got0, _ = scene.radiance(o, d, spp=3, spp_chunk=2)
    assert same(got0, query(scene, o, d, spp=3, spp_chunk=2))
    nxt, _ = scene.radiance(o, d, stream_ids=ids, spp=3, spp_chunk=2, spp_offset=3, prev_count=1, prev=got)
    assert same(nxt, query(scene, o, d, ids=ids, spp=3, spp_chunk=2, spp_offset=3, prev_count=1, prev=ref))
    e, st = scene.radiance(np.zeros((0, 3), f32), np.zeros((0, 3), f32))
    assert e.shape == (0, 3) and st["rays"] == 0


def test_overlapping_buffers_are_refused_and_left_alone(mcpt, ctx):
    import torch
    scene = ctx.scene("scene01")
    n = 1024
    o, d = ctx.rays("scene01", n)
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
            scene.radiance_device(n, O, D, **kw)
        assert e.value.code == -1 and "overlap" in str(e.value), kw
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
    assert scene.trace_stats()["rays"] == 0
    # adjacent, not overlapping: accepted
    scene.radiance_device(n, O, D, FREE, S, spp=2)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert same(got[7 * n:11 * n].reshape(n, 4)[:, :3], query(scene, o, d, spp=2))
    assert np.array_equal(got[:7 * n].view(np.uint32), before[:7 * n].view(np.uint32))
    assert (got[11 * n:] == f32(SENT)).all()


def test_a_scene_that_renders_in_quinengine_mode_answers_as_any_other(mcpt, ctx):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    scene.render(mcpt.RenderParams.for_quinengine(width=32, height=24))
    o, d = ctx.rays("scene01", 2000)
    assert same(query(scene, o, d, spp=2), query(ctx.scene("scene01"), o, d, spp=2))


def test_a_two_replica_scene_answers_as_the_single_device_scene(mcpt, ctx):
    o, d = ctx.rays("scene01", 2000)
    tr = mcpt.Tracer()
    try:
        tr.initialize([0, 0])
        multi = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
        assert multi.info()["n_devices"] == 2
        got = query(multi, o, d, spp=3, spp_chunk=2)
        st = multi.trace_stats()
    finally:
        tr.initialize([0])
    single = ctx.scene("scene01")
    single.trace_stats()
    assert same(got, query(single, o, d, spp=3, spp_chunk=2))
    rs = single.trace_stats()
    for k in COUNTERS:
        assert st[k] == rs[k], (k, st[k], rs[k])


def test_render_stats_and_radiance_stats_do_not_touch_each_other(mcpt, ctx):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    p = mcpt.RenderParams(width=64, height=48, spp=4, spp_chunk=2)
    img0, st0 = scene.render(p)
    z = scene.trace_stats()                                            # after a render alone: zeros
    assert all(z[k] == 0 for k in COUNTERS + ("stack_spills",))
    o, d = ctx.rays("scene01", 2000)
    ref = query(ctx.scene("scene01"), o, d, spp=2)
    ctx.scene("scene01").trace_stats()
    query(ctx.scene("scene01"), o, d, spp=2)
    rs = ctx.scene("scene01").trace_stats()
    assert same(query(scene, o, d, spp=2), ref)
    img1, st1 = scene.render(p)                                        # the query still unread
    assert same(img0, img1)
    for k in COUNTERS + ("renders",):
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    st = scene.trace_stats()                                           # and the render left the query's alone
    for k in COUNTERS:
        assert st[k] == rs[k], (k, st[k], rs[k])
