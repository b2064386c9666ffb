"""Ambient-occlusion queries (mcpt_ao_device, mcpt_render_ao_device and their host forms)
on torch tensors, against the numpy / oracle restatement of tests/_ao_ref.py and against
mcpt_occluded_device fed the restatement's rays: the output's bits and the counters are
equal, for the LDS and the global-memory layout, every radius, bias and stream id, every
batch shape and scheduling field at which the dealing of (point, samples) units to
workgroups, waves and lanes takes another path, the running mean, the pixel form and the
plumbing (reserve, streams, stats, overlap checks, the shared spill area).

Every output tensor carries 64 guard elements behind it, checked after every query.
"""
import numpy as np
import pytest

import _ao_ref as R
from _aov_ref import primary_rays
from _radiance_q import CONFIGS, VISITS, same

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 64, 48
GUARD = 64
SENT = -123.5
KEYS = ["scene01", "scene01-global", "scene03"]
WALK = ("rays",) + VISITS


class Ctx:
    """scenes, oracle scenes, frames and reference flags, each made once and left alone"""

    def __init__(self, mcpt, oracle_mod):
        self.mcpt, self.oracle = mcpt, oracle_mod
        self._scene, self._oscene, self._frame, self._flags = {}, {}, {}, {}

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

    def boxes(self, key):
        return int(self.scene(key).info()["node_boxes"])

    def cam(self, key):
        return dict(eye=CONFIGS[key][2], direction=CONFIGS[key][3])

    def rparams(self, key, **kw):
        c = self.cam(key)
        return self.mcpt.RenderParams(**{**dict(width=W, height=H, spp=2, eye=c["eye"], direction=c["direction"]), **kw})

    def frame(self, key, spp, spp_offset=0, w=W, h=H):
        k = (key, spp, spp_offset, w, h)
        if k not in self._frame:
            self._frame[k] = R.frame(self.oracle, self.oscene(key), w, h, spp, spp_offset, node_boxes=self.boxes(key),
                                     **self.cam(key))
        return self._frame[k]

    def hits(self, key):
        """the hit points of the 64 x 48, 1-spp primary rays, their unflipped shading normals
        and pixel indices"""
        fr = self.frame(key, 1)
        ok = fr["hit"][0]
        return (np.ascontiguousarray(fr["hp"][0][ok]), np.ascontiguousarray(fr["nrm"][0][ok]),
                np.nonzero(ok.ravel())[0].astype(np.uint32))

    def many(self, key, n=3000):
        """n hit points of the 2-spp frame, their shading normals turned towards the viewer (a
        real mix of occluded and open samples on every scene) and ids of their own: the
        scheduling tests' points"""
        fr = self.frame(key, 2)
        ok = fr["hit"].ravel()
        sel = np.nonzero(ok)[0][:n]
        assert sel.shape[0] == n
        nrm = np.where(fr["flip"].ravel()[sel][:, None], -fr["nrm"].reshape(-1, 3)[sel], fr["nrm"].reshape(-1, 3)[sel])
        return (np.ascontiguousarray(fr["hp"].reshape(-1, 3)[sel]), np.ascontiguousarray(nrm, f32),
                (sel.astype(np.uint32) * np.uint32(7) + np.uint32(11)))

    def flags(self, tag, key, p, nrm, ids, spp, spp_offset, radius, bias=0.0):
        """(rays o, d (spp, n, 3), occluded (spp, n)) of the restatement, cached under tag"""
        k = (tag, key, spp, spp_offset, float(radius), float(bias))
        if k not in self._flags:
            o, d = R.point_rays(self.oracle, p, nrm, ids, spp, spp_offset, bias=bias)
            self._flags[k] = (o, d, R.occluded(self.oracle, self.oscene(key), o, d, radius, self.boxes(key)))
        return self._flags[k]


@pytest.fixture(scope="module")
def ctx(mcpt, oracle_mod):
    return Ctx(mcpt, oracle_mod)


def _out(torch, n, prev):
    out = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    if prev is not None:
        out[:n] = torch.from_numpy(np.ascontiguousarray(prev, f32).ravel()).cuda()
    return out


def _read(out, n):
    h = out.cpu().numpy()
    assert (h[n:] == f32(SENT)).all(), "guard behind the output overwritten"
    return h[:n].copy()


def ao_points(scene, p, nrm, ids=None, prev=None, stream=None, **params):
    """Scene.ao_device on fresh torch tensors -> (n,) float32; the guard checked"""
    import torch
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, f32).reshape(-1, 3)
    n = p.shape[0]
    d_p, d_n = torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32)).cuda() if ids is not None else None
    out = _out(torch, n, prev)
    torch.cuda.synchronize()
    scene.ao_device(n, d_p.data_ptr(), d_n.data_ptr(), out.data_ptr(), d_s.data_ptr() if d_s is not None else 0,
                    stream.cuda_stream if stream is not None else 0, **params)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return _read(out, n)


def ao_frame(scene, rp, prev=None, **ao):
    """Scene.render_ao_device on a fresh torch tensor -> (H, W) float32; the guard checked"""
    import torch
    n = int(rp.width) * int(rp.height)
    out = _out(torch, n, prev)
    torch.cuda.synchronize()
    scene.render_ao_device(rp, out.data_ptr(), **ao)
    torch.cuda.synchronize()
    return _read(out, n).reshape(int(rp.height), int(rp.width))


def occluded_flags(scene, o, d, radius, **params):
    """Scene.occluded_device over rays (..., 3) with t_max = radius -> bool array, counters of the call"""
    import torch
    shape = o.shape[:-1]
    o = np.ascontiguousarray(o.reshape(-1, 3))
    d = np.ascontiguousarray(d.reshape(-1, 3))
    n = o.shape[0]
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    occ = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene.trace_stats()
    scene.occluded_device(n, d_o.data_ptr(), d_d.data_ptr(), occ.data_ptr(), t_max=radius, **params)
    st = scene.trace_stats()
    h = occ.cpu().numpy()
    assert (h[n:] == 0xAB).all()
    return h[:n].reshape(shape).astype(bool), st


def mean_of(occ, prev=None, prev_count=0):
    return R.value((~occ).sum(axis=0), occ.shape[0], prev, prev_count)


# ---- 1. the point form equals the restatement ----------------------------------------

@pytest.mark.parametrize("case", ["default-bias", "bias-0.05", "permuted-ids", "facing-normals"])
@pytest.mark.parametrize("key", KEYS)
def test_point_form_equals_the_restatement(ctx, key, case):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key)
    bias = 0.05 if case == "bias-0.05" else 0.0
    if case == "permuted-ids":
        ids = ids[np.random.default_rng(5).permutation(ids.shape[0])]
    if case == "facing-normals":       # (turned towards the viewer: scene01's mostly point away from it)
        flip = ctx.frame(key, 1)["flip"][0][ctx.frame(key, 1)["hit"][0]]
        nrm = np.where(flip[:, None], -nrm, nrm).astype(f32)
    shares = []
    for radius in (2.0, 8.0, 0.0):
        _, _, occ = ctx.flags(case, key, p, nrm, ids, 3, 5, radius, bias)
        got = ao_points(scene, p, nrm, ids, spp=3, spp_offset=5, radius=radius, bias=bias)
        assert same(got, mean_of(occ)), (key, case, radius, np.nonzero(got != mean_of(occ))[0][:10])
        shares.append(float(occ.mean()))
    print(key, case, "occluded shares at radius 2, 8, unbounded:", shares)
    assert shares[0] < shares[1] <= shares[2] and 0 < shares[0] and shares[1] < 1
    if case == "default-bias":
        # without the stream ids the id is the point's index; through the host entry too
        _, _, occ = ctx.flags("index-ids", key, p, nrm, np.arange(p.shape[0], dtype=np.uint32), 3, 5, 2.0)
        assert same(ao_points(scene, p, nrm, None, spp=3, spp_offset=5, radius=2.0), mean_of(occ))
        host, st = scene.ao(p, nrm, spp=3, spp_offset=5, radius=2.0)
        assert same(host, mean_of(occ))
        assert st["rays"] == st["paths"] == st["shades"] == 3 * p.shape[0]


# ---- 2. ... and the existing any-hit entry fed the same rays ---------------------------

@pytest.mark.parametrize("key", KEYS)
def test_point_form_equals_occluded_device_and_counts_its_walks(ctx, key):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key)
    n = p.shape[0]
    for radius in (2.0, 0.0):
        o, d, occ = ctx.flags("default-bias", key, p, nrm, ids, 3, 5, radius)
        flags, ref = occluded_flags(scene, o, d, radius)
        assert np.array_equal(flags, occ)
        scene.trace_stats()
        got = ao_points(scene, p, nrm, ids, spp=3, spp_offset=5, radius=radius)
        st = scene.trace_stats()
        assert same(got, mean_of(flags))
        for k in WALK:
            assert st[k] == ref[k], (key, radius, k, st[k], ref[k])
        assert st["rays"] == st["paths"] == st["shades"] == 3 * n
        lean = ao_points(scene, p, nrm, ids, spp=3, spp_offset=5, radius=radius, lean=1)
        st = scene.trace_stats()
        assert same(lean, got)
        assert st["rays"] == st["paths"] == st["shades"] == 3 * n
        assert all(st[k] == 0 for k in VISITS), st


# ---- 3. scheduling never changes a bit -----------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_batch_shapes_and_scheduling_fields_give_the_same_bits(ctx, key):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.many(key)
    _, _, occ = ctx.flags("many", key, p, nrm, ids, 5, 5, 2.0)
    assert 0.05 < occ.mean() < 0.95
    for n in (1, 63, 64, 65, 1025):
        for spp in (1, 5):
            got = ao_points(scene, p[:n], nrm[:n], ids[:n], spp=spp, spp_offset=5, radius=2.0)
            assert same(got, mean_of(occ[:spp, :n])), (key, n, spp)
    ref = mean_of(occ)
    for wg in (1, 3):
        for refill in (1, 64):
            for unit in (1, 2, 0):
                scene.trace_stats()
                got = ao_points(scene, p, nrm, ids, spp=5, spp_offset=5, radius=2.0, workgroups=wg, refill=refill,
                                unit_samples=unit, lean=1)
                assert same(got, ref), (key, wg, refill, unit)
                st = scene.trace_stats()
                assert st["rays"] == st["paths"] == st["shades"] == 5 * p.shape[0]
    # a unit of all the samples (the lane owns the point), a longer one, one that does not divide them
    for unit in (5, 64, 3):
        assert same(ao_points(scene, p, nrm, ids, spp=5, spp_offset=5, radius=2.0, unit_samples=unit), ref), unit


# ---- 4. the running mean -------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_chained_calls_continue_the_running_mean(ctx, key):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key)
    _, _, occ = ctx.flags("chain", key, p, nrm, ids, 4, 0, 2.0)
    first = ao_points(scene, p, nrm, ids, spp=2, spp_offset=0, radius=2.0)
    assert same(first, mean_of(occ[:2]))
    want = mean_of(occ[2:], prev=mean_of(occ[:2]), prev_count=1)
    for unit in (0, 2):                     # the finishing kernel's blend, and the owning lane's
        got = ao_points(scene, p, nrm, ids, prev=first, spp=2, spp_offset=2, prev_count=1, radius=2.0,
                        unit_samples=unit)
        assert same(got, want), unit
    assert not same(want, mean_of(occ[2:]))
    host, _ = scene.ao(p, nrm, ids, prev=first, spp=2, spp_offset=2, prev_count=1, radius=2.0)
    assert same(host, want)


# ---- 5. the pixel form equals the restatement -----------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_pixel_form_equals_the_restatement(ctx, key):
    scene = ctx.scene(key)
    fr = ctx.frame(key, 2)
    hits = int(fr["hit"].sum())
    rp = ctx.rparams(key)
    ac, _ = scene.render_aov(rp)
    for radius in (4.0, 0.0):
        want, occ = R.pixel_reference(ctx.oracle, ctx.oscene(key), fr, radius, ctx.boxes(key))
        scene.trace_stats()
        got = ao_frame(scene, rp, radius=radius)
        st = scene.trace_stats()
        assert same(got, want), (key, radius, np.argwhere(got != want)[:10])
        assert st["rays"] == W * H * 2 + hits and st["paths"] == W * H * 2 and st["shades"] == hits
        assert (got[ac[..., 3] == 0] == 1.0).all()
        # scheduling, lean and the host entry: the same bits
        for kw in (dict(lean=1), dict(unit_samples=2, workgroups=2, refill=1), dict(unit_samples=1, lean=1, refill=64)):
            assert same(ao_frame(scene, rp, radius=radius, **kw), want), kw
        st = scene.trace_stats()
        assert st["rays"] == 3 * (W * H * 2 + hits) and st["shades"] == 3 * hits
        host, hs = scene.render_ao(rp, radius=radius)
        assert same(host, want) and hs["rays"] == W * H * 2 + hits and hs["shades"] == hits
        assert scene.trace_stats()["rays"] == 0          # the host entry leaves the device entries' block alone
    assert 0.05 < occ[fr["hit"]].mean() < 1.0


def test_pixel_form_on_a_frame_of_partial_tiles_and_its_running_mean(ctx):
    key, w, h = "scene01", 37, 21
    scene = ctx.scene(key)
    fr = ctx.frame(key, 4, 0, w, h)
    half = [{k: v[a:b] for k, v in fr.items()} for a, b in ((0, 2), (2, 4))]
    first, _ = R.pixel_reference(ctx.oracle, ctx.oscene(key), half[0], 4.0)
    want, _ = R.pixel_reference(ctx.oracle, ctx.oscene(key), half[1], 4.0, prev=first, prev_count=1)
    for tile in (8, 4, 16):
        got = ao_frame(scene, ctx.rparams(key, width=w, height=h, tile=tile), radius=4.0)
        assert same(got, first), tile
    for unit in (0, 2):                     # one lane per sample and ao_finish, and one lane per pixel
        got = ao_frame(scene, ctx.rparams(key, width=w, height=h, spp_offset=2, prev_count=1), prev=first, radius=4.0,
                       unit_samples=unit)
        assert same(got, want), unit


# ---- 6. the pixel form against the point form -----------------------------------------

def test_pixel_form_is_the_point_form_at_its_hits_where_no_sample_flips(ctx):
    key, s = "scene03", 3
    scene = ctx.scene(key)
    fr = ctx.frame(key, 1, s)
    ok = fr["hit"][0] & ~fr["flip"][0]
    assert ok.mean() >= 0.99
    pix = np.nonzero(ok.ravel())[0].astype(np.uint32)
    frame = ao_frame(scene, ctx.rparams(key, spp=1, spp_offset=s), radius=4.0)
    points = ao_points(scene, fr["hp"][0][ok], fr["nrm"][0][ok], pix, spp=1, spp_offset=s, radius=4.0)
    assert same(frame.ravel()[pix], points)
    assert 0.05 < 1.0 - points.mean() < 0.95


# ---- 7. the 70k-triangle mesh (global layout) ------------------------------------------

def test_point_form_on_the_bunny_mesh_equals_occluded_device(ctx):
    import torch
    mcpt = ctx.mcpt
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("cornell_bunny70k")))
    assert int(scene.info()["node_boxes"]) == 1
    # points: the closest hits of a frame's primary rays (the device's own); normals: back along the rays
    o, d = primary_rays(ctx.oracle, W, H, 1)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.full((W * H,), -7, dtype=torch.int32, device="cuda")
    hit = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    scene.trace_device(W * H, d_o.data_ptr(), d_d.data_ptr(), tri.data_ptr(), hit.data_ptr())
    torch.cuda.synchronize()
    sel = np.nonzero(tri.cpu().numpy() >= 0)[0][:2000]
    assert sel.shape[0] == 2000
    t = hit.cpu().numpy()[sel, 2]
    p = (o[sel] + t[:, None] * d[sel]).astype(f32)
    nrm = (-d[sel]).astype(f32)
    ids = sel.astype(np.uint32)
    for radius in (2.0, 0.0):
        ro, rd = R.point_rays(ctx.oracle, p, nrm, ids, 2, 1)
        flags, ref = occluded_flags(scene, ro, rd, radius)
        scene.trace_stats()
        got = ao_points(scene, p, nrm, ids, spp=2, spp_offset=1, radius=radius)
        st = scene.trace_stats()
        assert same(got, mean_of(flags)), radius
        for k in WALK:
            assert st[k] == ref[k], (radius, k, st[k], ref[k])
        assert same(ao_points(scene, p, nrm, ids, spp=2, spp_offset=1, radius=radius, lean=1, unit_samples=1), got)
        assert 0.02 < flags.mean() < 0.98, flags.mean()


# ---- 8. housekeeping -------------------------------------------------------------------

def test_reserve_and_no_allocation_afterwards(mcpt, ctx):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))      # a scene that has run no query
    p, nrm, ids = ctx.hits("scene01")
    n = p.shape[0]
    _, _, occ = ctx.flags("default-bias", "scene01", p, nrm, ids, 3, 5, 2.0)
    rp = ctx.rparams("scene01")
    want_px, _ = R.pixel_reference(ctx.oracle, ctx.oscene("scene01"), ctx.frame("scene01", 2), 4.0)
    d_p, d_n = torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda()
    d_s = torch.from_numpy(ids.view(np.int32)).cuda()
    out = torch.full((n,), SENT, dtype=torch.float32, device="cuda")
    opx = torch.full((W * H,), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.reserve_ao(W * H)
    free0 = scene.plan(rp)["device_free_bytes"]
    for unit in (0, 3):                                                # the first pair of calls, and a second
        scene.ao_device(n, d_p.data_ptr(), d_n.data_ptr(), out.data_ptr(), d_s.data_ptr(), spp=3, spp_offset=5,
                        radius=2.0, unit_samples=unit)
        scene.render_ao_device(rp, opx.data_ptr(), radius=4.0, unit_samples=unit)
        torch.cuda.synchronize()
        assert scene.plan(rp)["device_free_bytes"] == free0
        assert same(out.cpu().numpy(), mean_of(occ))
        assert same(opx.cpu().numpy().reshape(H, W), want_px)
    assert scene.trace_stats()["paths"] == 2 * (3 * n + 2 * W * H)
    assert scene.trace_stats()["rays"] == 0                            # read and reset
    scene.ao_device(0, 0, 0, 0)                                        # n = 0 is a no-op
    assert scene.trace_stats()["rays"] == 0


def test_query_on_a_torch_stream(ctx):
    import torch
    scene = ctx.scene("scene01")
    p, nrm, ids = ctx.hits("scene01")
    _, _, occ = ctx.flags("default-bias", "scene01", p, nrm, ids, 3, 5, 2.0)
    got = ao_points(scene, p, nrm, ids, stream=torch.cuda.Stream(), spp=3, spp_offset=5, radius=2.0)
    assert same(got, mean_of(occ))


def test_overlapping_buffers_are_refused_and_left_alone(mcpt, ctx):
    import torch
    scene = ctx.scene("scene01")
    p, nrm, ids = ctx.hits("scene01")
    n = 1024
    p, nrm, ids = p[:n], nrm[:n], ids[:n]
    buf = torch.full((16 * n,), SENT, dtype=torch.float32, device="cuda")
    buf[:3 * n] = torch.from_numpy(p.ravel()).cuda()
    buf[3 * n:6 * n] = torch.from_numpy(nrm.ravel()).cuda()
    buf[6 * n:7 * n] = torch.from_numpy(ids.view(f32)).cuda()
    torch.cuda.synchronize()
    before = buf.cpu().numpy().copy()
    base = buf.data_ptr()
    P, N, S, FREE = base, base + 12 * n, base + 24 * n, base + 28 * n
    scene.trace_stats()
    for out_ptr in (P + 8, N - 4, N, S - 4, S + 4 * n - 4):
        with pytest.raises(mcpt.McptError) as e:
            scene.ao_device(n, P, N, out_ptr, S)
        assert e.value.code == -1 and "overlap" in str(e.value), out_ptr - base
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
    assert scene.trace_stats()["rays"] == 0
    # adjacent, not overlapping: accepted; without the ids their place is free
    scene.ao_device(n, P, N, FREE, S, spp=3, spp_offset=5, radius=2.0)
    scene.ao_device(n, P, N, FREE + 4 * n, 0, spp=3, spp_offset=5, radius=2.0)
    torch.cuda.synchronize()
    _, _, occ = ctx.flags("sub1024", "scene01", p, nrm, ids, 3, 5, 2.0)
    got = buf.cpu().numpy()
    assert same(got[7 * n:8 * n], mean_of(occ))
    assert np.array_equal(got[:7 * n].view(np.uint32), before[:7 * n].view(np.uint32))
    assert (got[9 * n:] == f32(SENT)).all()


def test_queries_leave_the_render_stats_alone_and_share_the_spill_area(mcpt, ctx):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), layout="global")
    rp = mcpt.RenderParams(width=W, height=H, spp=4, spp_chunk=2)
    img0, st0 = scene.render(rp)
    z = scene.trace_stats()                                            # after a render alone: zeros
    assert all(z[k] == 0 for k in WALK + ("paths", "shades"))
    p, nrm, ids = ctx.hits("scene01-global")
    _, _, occ = ctx.flags("default-bias", "scene01-global", p, nrm, ids, 3, 5, 0.0)
    assert same(ao_points(scene, p, nrm, ids, spp=3, spp_offset=5), mean_of(occ))
    want_px, _ = R.pixel_reference(ctx.oracle, ctx.oscene("scene01"), ctx.frame("scene01-global", 2), 0.0, 1)
    assert same(ao_frame(scene, ctx.rparams("scene01-global")), want_px)
    img1, st1 = scene.render(rp)                                       # the queries still unread
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
    for k in ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades", "renders"):
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    st = scene.trace_stats()                                           # and the render left the queries' alone
    assert st["paths"] == 3 * p.shape[0] + 2 * W * H
