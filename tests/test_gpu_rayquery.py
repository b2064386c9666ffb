"""Device ray queries (mcpt_trace_device, mcpt_occluded_device, mcpt_occluded)
on torch tensors, against mcpt_intersect (Scene.intersect) and the CPU oracle's
ordered walk: triangle ids, the bits of (beta, gamma, t) and the traversal
counters are equal, for the LDS and the global-memory layout, per-ray t_max,
the any-hit early exit, every batch shape at which the dealing of rays to
workgroups and waves takes another path, the lean kernels and the plumbing
(reserve, streams, stats, overlap checks, replicas).

Rays: the adversarial families of tests/_raysets.py, seed 23.  Every output
tensor carries 64 guard elements behind it, checked after every query.
"""
import numpy as np
import pytest

from _raysets import ray_sets

pytestmark = pytest.mark.gpu

N = 100_000
FLT_MAX = 3.402823466e38
COUNTERS = ("rays", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests")
GUARD = 64
SENT_I, SENT_F, SENT_B = -77, -123.5, 0xAB
CONFIGS = {                                   # key -> (scene, layout, kd_build)
    "scene01": ("scene01", "auto", "reference"),
    "scene01-global": ("scene01", "global", "reference"),
    "scene03": ("scene03", "auto", "reference"),
    "scene01-sah": ("scene01", "auto", "sah"),
    "bunny": ("cornell_bunny70k", "auto", "reference"),
}


class Ctx:
    """scenes, oracle scenes, ray sets and Scene.intersect references, each made once"""

    def __init__(self, mcpt, oracle_mod):
        self.mcpt, self.oracle = mcpt, oracle_mod
        self._scene, self._oscene, self._rays, self._ref = {}, {}, {}, {}

    def scene(self, key):
        if key not in self._scene:
            name, layout, kd = CONFIGS[key]
            self._scene[key] = self.mcpt.Scene(self.mcpt.ObjModel(self.mcpt.scene_path(name)), layout=layout,
                                               kd_build=kd)
        return self._scene[key]

    def oscene(self, key):
        name, _, kd = CONFIGS[key]
        if (name, kd) not in self._oscene:
            self._oscene[(name, kd)] = self.oracle.Scene(self.mcpt.scene_path(name), kd_build=kd)
        return self._oscene[(name, kd)]

    def rays(self, key, n=N):
        """ray_sets(oracle scene, n, seed 23); the tree only picks the split-plane origins"""
        name, _, kd = CONFIGS[key]
        if (name, kd, n) not in self._rays:
            self._rays[(name, kd, n)] = ray_sets(self.oscene(key), n, seed=23)
        return self._rays[(name, kd, n)]

    def subset(self, key, n):
        """n rays spread over all families of the scene's 100 000"""
        o, d = self.rays(key)
        sel = np.arange(n) * (o.shape[0] // n)
        return np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])

    def ref(self, key, tag, o, d, t_max=FLT_MAX):
        """Scene.intersect of the rays (tag names them), cached"""
        k = (key, tag, float(t_max))
        if k not in self._ref:
            self._ref[k] = self.scene(key).intersect(o, d, t_max=t_max)
        return self._ref[k]


@pytest.fixture(scope="module")
def ctx(mcpt, oracle_mod):
    return Ctx(mcpt, oracle_mod)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _guarded(torch, n, per, dtype, sentinel):
    return torch.full((n * per + GUARD,), sentinel, dtype=dtype, device="cuda")


def trace(scene, o, d, tm=None, want_hit=True, stream=None, **params):
    """Scene.trace_device on fresh torch tensors -> (tri, hit or None); guards checked.
    tm: the per-ray t_max array (None: d_t_max = NULL, params' scalar t_max for every ray)"""
    import torch
    n = o.shape[0]
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(tm, np.float32)).cuda() if tm is not None else None
    tri = _guarded(torch, n, 1, torch.int32, SENT_I)
    hit = _guarded(torch, n, 3, torch.float32, SENT_F) if want_hit else None
    torch.cuda.synchronize()
    scene.trace_device(n, d_o.data_ptr(), d_d.data_ptr(), tri.data_ptr(), hit.data_ptr() if want_hit else 0,
                       d_t.data_ptr() if d_t is not None else 0, stream.cuda_stream if stream is not None else 0,
                       **params)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    tri_h = tri.cpu().numpy()
    assert (tri_h[n:] == SENT_I).all(), "guard behind tri overwritten"
    hit_h = None
    if want_hit:
        hit_h = hit.cpu().numpy()
        assert (hit_h[3 * n:] == np.float32(SENT_F)).all(), "guard behind hit overwritten"
        hit_h = hit_h[:3 * n].reshape(n, 3)
    return tri_h[:n], hit_h


def occluded(scene, o, d, tm=None, **params):
    import torch
    n = o.shape[0]
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(tm, np.float32)).cuda() if tm is not None else None
    occ = _guarded(torch, n, 1, torch.uint8, SENT_B)
    torch.cuda.synchronize()
    scene.occluded_device(n, d_o.data_ptr(), d_d.data_ptr(), occ.data_ptr(), d_t.data_ptr() if d_t is not None else 0,
                          **params)
    torch.cuda.synchronize()
    occ_h = occ.cpu().numpy()
    assert (occ_h[n:] == SENT_B).all(), "guard behind occluded overwritten"
    return occ_h[:n]


def assert_same_hits(tri, hit, ref_tri, ref_hit, what=""):
    assert np.array_equal(tri, ref_tri), (what, np.nonzero(tri != ref_tri)[0][:10])
    if hit is not None:
        assert np.array_equal(_bits(hit), _bits(ref_hit)), (what, "hit bits")
        assert (hit[tri < 0] == 0).all(), (what, "a miss reports zeros")


def assert_counters(st, ref, what=""):
    for k in COUNTERS:
        assert st[k] == ref[k], (what, k, st[k], ref[k])


def three_t_max(n):
    return np.array([FLT_MAX, 8.0, 4.0], np.float32)[np.arange(n) % 3]


# ---- 1. closest hit = mcpt_intersect = the oracle ------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global", "scene03", "scene01-sah"])
def test_closest_hit_equals_intersect_and_the_oracle_walk(ctx, key):
    scene = ctx.scene(key)
    boxes = int(scene.info()["node_boxes"])
    assert boxes == (0 if key in ("scene01", "scene01-sah") else 1)
    o, d = ctx.rays(key)
    scene.trace_stats()                                   # a fresh record
    tri, hit = trace(scene, o, d)
    st = scene.trace_stats()
    rt, rh, rs = ctx.ref(key, "all", o, d)
    assert_same_hits(tri, hit, rt, rh, key)
    assert_counters(st, rs, key)
    assert st["rays"] == o.shape[0]
    tk, gk, hk, ck = ctx.oscene(key).intersect(o, d, ctx.oracle.KD_ORDERED, node_boxes=boxes, threads=8)
    assert np.array_equal(tri, tk)
    hit_k = np.where(tk[:, None] >= 0, hk[:, :3], 0.0).astype(np.float32)
    assert np.array_equal(_bits(hit), _bits(hit_k))
    for k in COUNTERS[1:]:
        assert st[k] == ck[k], (k, st[k], ck[k])
    assert 0.3 < (tri >= 0).mean() < 1.0


def test_closest_hit_on_the_bunny_mesh_equals_intersect(ctx):
    scene = ctx.scene("bunny")
    o, d = ctx.rays("bunny")
    scene.trace_stats()
    tri, hit = trace(scene, o, d)
    st = scene.trace_stats()
    rt, rh, rs = ctx.ref("bunny", "all", o, d)
    assert_same_hits(tri, hit, rt, rh)
    assert_counters(st, rs)


# ---- 2. per-ray t_max ----------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene03"])
def test_per_ray_t_max_equals_intersect_per_class(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.rays(key)
    n = o.shape[0]
    tm = three_t_max(n)
    scene.trace_stats()
    tri, hit = trace(scene, o, d, tm=tm)
    st = scene.trace_stats()
    total = dict.fromkeys(COUNTERS, 0)
    for cls, value in enumerate((FLT_MAX, 8.0, 4.0)):
        sel = np.arange(n) % 3 == cls
        rt, rh, rs = ctx.ref(key, f"class{cls}", np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel]),
                             t_max=value)
        assert_same_hits(tri[sel], hit[sel], rt, rh, (key, value))
        frac = float((rt >= 0).mean())
        print(key, "t_max", value, "hit fraction", frac)
        assert 0.2 < frac <= 1.0, (value, frac)
        for k in COUNTERS:
            total[k] += rs[k]
    assert_counters(st, total, key)
    # the scalar form: no per-ray array, params' t_max for every ray
    tri4, hit4 = trace(scene, o, d, t_max=4.0)
    st4 = scene.trace_stats()
    rt, rh, rs = ctx.ref(key, "all", o, d, t_max=4.0)
    assert_same_hits(tri4, hit4, rt, rh, (key, "scalar 4.0"))
    assert_counters(st4, rs, (key, "scalar 4.0"))


# ---- 3. any hit ----------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene03"])
def test_any_hit_is_the_closest_hit_flag_with_an_early_exit(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.rays(key)
    n = o.shape[0]
    tm = three_t_max(n)
    scene.trace_stats()
    tri, _ = trace(scene, o, d, tm=tm)
    st_c = scene.trace_stats()
    occ = occluded(scene, o, d, tm=tm)
    st_a = scene.trace_stats()
    assert np.array_equal(occ, (tri >= 0).astype(np.uint8))
    occ_h, st_h = scene.occluded(o, d, t_max=tm)
    assert np.array_equal(occ_h, occ)
    assert scene.trace_stats()["rays"] == 0               # the host entry counts apart
    for st in (st_a, st_h):
        assert st["rays"] == st_c["rays"] == n
        for k in COUNTERS[1:]:
            assert st[k] <= st_c[k], (k, st[k], st_c[k])
    assert_counters(st_h, st_a, "host entry")
    print(key, "tri_tests any / closest", st_a["tri_tests"], st_c["tri_tests"])
    if key == "scene01":
        assert st_a["tri_tests"] < st_c["tri_tests"]      # the early exit exists
    # nothing within reach: no early exit, the closest-hit walk and its counters
    tri0, _ = trace(scene, o, d, t_max=1e-30)
    st_c0 = scene.trace_stats()
    occ0 = occluded(scene, o, d, t_max=1e-30)
    st_a0 = scene.trace_stats()
    assert (tri0 == -1).all() and not occ0.any()
    assert_counters(st_a0, st_c0, "t_max 1e-30")
    occ_s, st_s = scene.occluded(o, d, t_max=1e-30)       # the host entry's scalar form
    assert not occ_s.any()
    assert_counters(st_s, st_c0, "host t_max 1e-30")


# ---- 4. shapes where dealing and refill can go wrong ---------------------------

@pytest.mark.parametrize("key", ["scene01", "scene03"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025])
def test_small_batches(ctx, key, n):
    scene = ctx.scene(key)
    o, d = ctx.subset(key, n)
    scene.trace_stats()
    tri, hit = trace(scene, o, d)
    st = scene.trace_stats()
    rt, rh, rs = ctx.ref(key, f"sub{n}", o, d)
    assert_same_hits(tri, hit, rt, rh, (key, n))
    assert_counters(st, rs, (key, n))
    occ = occluded(scene, o, d)
    assert np.array_equal(occ, (rt >= 0).astype(np.uint8))
    assert scene.trace_stats()["rays"] == n


@pytest.mark.parametrize("key", ["scene01", "scene03"])
@pytest.mark.parametrize("params", [dict(workgroups=1), dict(workgroups=3, refill=1), dict(workgroups=3, refill=64)],
                         ids=["1wg", "3wg-refill1", "3wg-refill64"])
def test_few_workgroups_refill_over_the_batch(ctx, key, params):
    """n = 5000: one workgroup refills every lane about five (LDS, 1024 lanes) or twenty (global,
    256 lanes) times; three workgroups own 1728, 1728 and 1544 rays"""
    scene = ctx.scene(key)
    o, d = ctx.subset(key, 5000)
    scene.trace_stats()
    tri, hit = trace(scene, o, d, **params)
    st = scene.trace_stats()
    rt, rh, rs = ctx.ref(key, "sub5000", o, d)
    assert_same_hits(tri, hit, rt, rh, (key, params))
    assert_counters(st, rs, (key, params))
    occ = occluded(scene, o, d, **params)
    assert np.array_equal(occ, (rt >= 0).astype(np.uint8))


def test_more_rays_than_resident_lanes(ctx):
    scene = ctx.scene("scene01")
    o, d = ctx.rays("scene01", 300_000)
    assert o.shape[0] > 256 * 1024
    scene.trace_stats()
    tri, hit = trace(scene, o, d)
    st = scene.trace_stats()
    rt, rh, rs = scene.intersect(o, d)
    assert_same_hits(tri, hit, rt, rh)
    assert_counters(st, rs)


# ---- 5. lean -------------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene03"])
def test_lean_queries_give_the_same_results_and_count_rays_only(ctx, key):
    scene = ctx.scene(key)
    o, d = ctx.rays(key)
    n = o.shape[0]
    tm = three_t_max(n)
    tri_ref, hit_ref = trace(scene, o, d, tm=tm)
    scene.trace_stats()
    tri, hit = trace(scene, o, d, tm=tm, lean=True)
    st = scene.trace_stats()
    assert_same_hits(tri, hit, tri_ref, hit_ref, key)
    assert st["rays"] == n
    for k in COUNTERS[1:] + ("stack_spills",):
        assert st[k] == 0, (k, st[k])
    occ = occluded(scene, o, d, tm=tm, lean=True)
    st = scene.trace_stats()
    assert np.array_equal(occ, (tri_ref >= 0).astype(np.uint8))
    assert st["rays"] == n and all(st[k] == 0 for k in COUNTERS[1:])


# ---- 6. plumbing ---------------------------------------------------------------

def test_no_hit_buffer_reserve_and_no_allocation_afterwards(mcpt, ctx):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))      # a scene that has run no query
    o, d = ctx.subset("scene01", 5000)
    rt, rh, _ = ctx.ref("scene01", "sub5000", o, d)
    p = mcpt.RenderParams(width=64, height=48, spp=4)
    n = o.shape[0]
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.full((n,), SENT_I, dtype=torch.int32, device="cuda")
    occ = torch.full((n,), SENT_B, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene.reserve_rays()
    free0 = scene.plan(p)["device_free_bytes"]
    for _ in range(2):                                                 # the first pair of calls, and a second
        tri.fill_(SENT_I)
        occ.fill_(SENT_B)
        scene.trace_device(n, d_o.data_ptr(), d_d.data_ptr(), tri.data_ptr())       # d_hit = NULL
        scene.occluded_device(n, d_o.data_ptr(), d_d.data_ptr(), occ.data_ptr())
        torch.cuda.synchronize()
        assert scene.plan(p)["device_free_bytes"] == free0
        assert np.array_equal(tri.cpu().numpy(), rt)
        assert np.array_equal(occ.cpu().numpy(), (rt >= 0).astype(np.uint8))
    assert scene.trace_stats()["rays"] == 4 * n
    assert scene.trace_stats()["rays"] == 0                            # read and reset
    # n = 0 is a no-op
    scene.trace_device(0, 0, 0, 0)
    scene.occluded_device(0, 0, 0, 0)
    assert scene.trace_stats()["rays"] == 0


def test_render_stats_and_ray_query_stats_do_not_touch_each_other(mcpt, ctx):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    p = mcpt.RenderParams(width=64, height=48, spp=4, spp_chunk=2)
    img0, st0 = scene.render(p)
    z = scene.trace_stats()                                            # after a render alone: zeros
    assert all(z[k] == 0 for k in COUNTERS + ("stack_spills",))
    o, d = ctx.subset("scene01", 5000)
    rt, rh, rs = ctx.ref("scene01", "sub5000", o, d)
    tri, hit = trace(scene, o, d)
    assert_same_hits(tri, hit, rt, rh)
    img1, st1 = scene.render(p)                                        # the query still unread
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
    for k in ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades", "renders"):
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    assert_counters(scene.trace_stats(), rs)                           # and the render left the query's alone


def test_query_on_a_torch_stream(ctx):
    import torch
    scene = ctx.scene("scene01")
    o, d = ctx.subset("scene01", 5000)
    rt, rh, rs = ctx.ref("scene01", "sub5000", o, d)
    scene.trace_stats()
    s = torch.cuda.Stream()
    tri, hit = trace(scene, o, d, stream=s)
    assert_same_hits(tri, hit, rt, rh)
    assert_counters(scene.trace_stats(), rs)


def test_overlapping_buffers_are_refused_and_left_alone(mcpt, ctx):
    import torch
    scene = ctx.scene("scene01")
    n = 1024
    o, d = ctx.subset("scene01", n)
    buf = torch.full((16 * n,), SENT_F, dtype=torch.float32, device="cuda")
    buf[:3 * n] = torch.from_numpy(o.ravel()).cuda()
    buf[3 * n:6 * n] = torch.from_numpy(d.ravel()).cuda()
    torch.cuda.synchronize()
    before = buf.cpu().numpy().copy()
    base = buf.data_ptr()
    O, D, FREE = base, base + 12 * n, base + 24 * n
    scene.trace_stats()
    cases = [dict(tri_ptr=O + 8), dict(tri_ptr=D + 12 * n - 4), dict(tri_ptr=FREE, hit_ptr=D),
             dict(tri_ptr=FREE, hit_ptr=FREE + 4 * n - 4), dict(tri_ptr=FREE + 8 * n, t_max_ptr=FREE + 12 * n - 4)]
    for kw in cases:
        with pytest.raises(mcpt.McptError) as e:
            scene.trace_device(n, O, D, **kw)
        assert e.value.code == -1 and "overlap" in str(e.value), kw
    for kw in (dict(occluded_ptr=O + 12 * n - 1), dict(occluded_ptr=D), dict(occluded_ptr=FREE, t_max_ptr=FREE - 4 * n + n)):
        with pytest.raises(mcpt.McptError) as e:
            scene.occluded_device(n, O, D, **kw)
        assert e.value.code == -1 and "overlap" in str(e.value), kw
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
    assert scene.trace_stats()["rays"] == 0
    # adjacent, not overlapping: accepted
    scene.trace_device(n, O, D, FREE, FREE + 4 * n)
    torch.cuda.synchronize()
    rt, rh, _ = ctx.ref("scene01", f"sub{n}", o, d)
    got = buf.cpu().numpy()
    assert np.array_equal(got[6 * n:7 * n].view(np.int32), rt)
    assert np.array_equal(_bits(got[7 * n:10 * n].reshape(n, 3)), _bits(rh))


def test_a_two_replica_scene_answers_as_the_single_device_scene(mcpt, ctx):
    tr = mcpt.Tracer()
    try:
        tr.initialize([0, 0])
        multi = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
        assert multi.info()["n_devices"] == 2
        o, d = ctx.subset("scene01", 5000)
        tm = three_t_max(5000)
        tri, hit = trace(multi, o, d, tm=tm)
        occ = occluded(multi, o, d, tm=tm)
        st = multi.trace_stats()
    finally:
        tr.initialize([0])
    single = ctx.scene("scene01")
    single.trace_stats()
    rt, rh = trace(single, o, d, tm=tm)
    rocc = occluded(single, o, d, tm=tm)
    assert_same_hits(tri, hit, rt, rh)
    assert np.array_equal(occ, rocc)
    assert_counters(st, single.trace_stats())
