"""Direct-lighting queries (mcpt_direct_device, mcpt_render_direct_device and their host
forms) on torch tensors, against the numpy / oracle restatement of tests/_direct_ref.py
and against the composed path -- the restatement's valid shadow rays sent through
mcpt_occluded_device with a per-ray t_max (and mcpt_trace_device for the pixel form's
primary rays), the flags combined in numpy: the output's bits and the counters are equal,
for the LDS and the global-memory layout, a scene of 1680 lights and a closed room, every
batch shape and scheduling field at which the dealing of (point, chunk) units takes
another path, every chunking, the running mean, the edge cases that form no ray, and the
plumbing (reserve, streams, stats, overlap checks, replicas).

Every output tensor carries 64 guard elements behind it, checked after every query.
"""
import numpy as np
import pytest

import _direct_ref as R
from _aov_ref import primary_rays
from _radiance_q import VISITS, same
from test_gpu_ao import ao_points

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 64, 48
GUARD = 64
SENT = -123.5
# key -> (scene, layout, eye, direction)
CONFIGS = {
    "scene01": ("scene01", "auto", (0.0, 5.0, 17.0), (0.0, 0.0, -1.0)),
    "scene01-global": ("scene01", "global", (0.0, 5.0, 17.0), (0.0, 0.0, -1.0)),
    "scene02": ("scene02", "auto", (0.0, 5.0, 23.0), (0.0, 0.0, -1.0)),
    "scene03": ("scene03", "auto", (0.0, 5.0, 4.0), (0.0, 0.5, -1.0)),
}
KEYS = list(CONFIGS)
WALK = ("rays",) + VISITS


class Ctx:
    """scenes, oracle scenes, light tables, frames and reference records, each made once and left alone"""

    def __init__(self, mcpt, oracle_mod):
        self.mcpt, self.oracle = mcpt, oracle_mod
        self._scene, self._oscene, self._table, self._pix, self._pts = {}, {}, {}, {}, {}

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

    def table(self, key):
        name = CONFIGS[key][0]
        if name not in self._table:
            self._table[name] = R.light_table(self.oscene(key))
        return self._table[name]

    def boxes(self, key):
        return int(self.scene(key).info()["node_boxes"])

    def cam(self, key):
        return dict(eye=CONFIGS[key][2], direction=CONFIGS[key][3])

    def rparams(self, key, **kw):
        c = self.cam(key)
        return self.mcpt.RenderParams(**{**dict(width=W, height=H, spp=3, eye=c["eye"], direction=c["direction"]), **kw})

    def pixels(self, key, spp, spp_offset=0, w=W, h=H):
        """(record, frame, visible) of the pixel form's samples"""
        k = (key, spp, spp_offset, w, h)
        if k not in self._pix:
            rec, fr = R.pixel_samples(self.oracle, self.oscene(key), self.table(key), w, h, spp, spp_offset,
                                      node_boxes=self.boxes(key), **self.cam(key))
            self._pix[k] = (rec, fr, R.visible(self.oracle, self.oscene(key), rec, self.boxes(key)))
        return self._pix[k]

    def hits(self, key, n=None):
        """the hit points of the 64 x 48, 1-spp primary rays, their shading normals turned towards
        the viewer and ids of their own (the first n of them)"""
        _, fr, _ = self.pixels(key, 1)
        ok = fr["hit"][0]
        nrm = np.where(fr["flip"][0][ok][:, None], -fr["nrm"][0][ok], fr["nrm"][0][ok]).astype(f32)
        ids = np.nonzero(ok.ravel())[0].astype(np.uint32) * np.uint32(7) + np.uint32(11)
        p = np.ascontiguousarray(fr["hp"][0][ok])
        n = p.shape[0] if n is None else n
        assert p.shape[0] >= n
        return p[:n], np.ascontiguousarray(nrm[:n]), ids[:n]

    def many(self, key, n=3000):
        """n hit points of the 2-spp frame, their shading normals turned towards the viewer and
        ids of their own: the scheduling tests' points"""
        _, fr, _ = self.pixels(key, 2)
        sel = np.nonzero(fr["hit"].ravel())[0][:n]
        assert sel.shape[0] == n
        nrm = np.where(fr["flip"].ravel()[sel][:, None], -fr["nrm"].reshape(-1, 3)[sel], fr["nrm"].reshape(-1, 3)[sel])
        return (np.ascontiguousarray(fr["hp"].reshape(-1, 3)[sel]), np.ascontiguousarray(nrm, f32),
                (sel.astype(np.uint32) * np.uint32(7) + np.uint32(11)))

    def points(self, tag, key, p, nrm, ids, spp, spp_offset=0, bias=0.0, seed=R.SEED):
        """(record, visible) of the point form's samples, cached under tag"""
        k = (tag, key, spp, spp_offset, float(bias), seed)
        if k not in self._pts:
            rec = R.point_samples(self.oracle, self.table(key), p, nrm, ids, spp, spp_offset, seed, bias)
            self._pts[k] = (rec, R.visible(self.oracle, self.oscene(key), rec, self.boxes(key)))
        return self._pts[k]


@pytest.fixture(scope="module")
def ctx(mcpt, oracle_mod):
    return Ctx(mcpt, oracle_mod)


def _out(torch, n, prev):
    out = torch.full((4 * n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    if prev is not None:
        old = np.zeros((n, 4), f32)
        old[:, :3] = np.asarray(prev, f32).reshape(n, 3)
        out[:4 * n] = torch.from_numpy(old.ravel()).cuda()
    return out


def _read(out, n):
    h = out.cpu().numpy()
    assert (h[4 * n:] == f32(SENT)).all(), "guard behind the output overwritten"
    h = h[:4 * n].reshape(n, 4)
    assert (h[:, 3] == 0).all() and not np.signbit(h[:, 3]).any()
    return np.ascontiguousarray(h[:, :3])


def direct_points(scene, p, nrm, ids=None, prev=None, stream=None, **params):
    """Scene.direct_device on fresh torch tensors -> (n, 3) float32; the guard and the fourth lane checked"""
    import torch
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, f32).reshape(-1, 3)
    n = p.shape[0]
    d_p, d_n = torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32)).cuda() if ids is not None else None
    out = _out(torch, n, prev)
    torch.cuda.synchronize()
    scene.direct_device(n, d_p.data_ptr(), d_n.data_ptr(), out.data_ptr(), d_s.data_ptr() if d_s is not None else 0,
                        stream.cuda_stream if stream is not None else 0, **params)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return _read(out, n)


def direct_frame(scene, rp, prev=None, **kw):
    """Scene.render_direct_device on a fresh torch tensor -> (H, W, 3) float32; the guard checked"""
    import torch
    n = int(rp.width) * int(rp.height)
    out = _out(torch, n, prev)
    torch.cuda.synchronize()
    scene.render_direct_device(rp, out.data_ptr(), **kw)
    torch.cuda.synchronize()
    return _read(out, n).reshape(int(rp.height), int(rp.width), 3)


def occluded_flags(scene, rec, **params):
    """Scene.occluded_device over the record's valid shadow rays with their own t_max -> occluded
    flags in the record's shape (False where no ray was formed), counters of the call"""
    import torch
    ok = rec["valid"].ravel()
    o = np.ascontiguousarray(rec["o"].reshape(-1, 3)[ok])
    d = np.ascontiguousarray(rec["d"].reshape(-1, 3)[ok])
    tm = np.ascontiguousarray(rec["t_max"].ravel()[ok])
    n = o.shape[0]
    flags = np.zeros(ok.shape[0], bool)
    scene.trace_stats()
    if n:
        d_o, d_d, d_t = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(tm).cuda()
        occ = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        scene.occluded_device(n, d_o.data_ptr(), d_d.data_ptr(), occ.data_ptr(), d_t.data_ptr(), **params)
        torch.cuda.synchronize()
        h = occ.cpu().numpy()
        assert (h[n:] == 0xAB).all()
        flags[ok] = h[:n].astype(bool)
    return flags.reshape(rec["valid"].shape), scene.trace_stats()


def value_of(ctx, key, rec, vis, chunk=0, illum=10.0, prev=None, prev_count=0):
    return R.value(R.contributions(ctx.table(key), rec, vis, illum), chunk, prev, prev_count)


# ---- 1. the point form: the restatement, the composed path, the counters ----------------

@pytest.mark.parametrize("key", KEYS)
def test_point_form_equals_the_restatement_and_the_composed_path(ctx, key):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key)
    n, spp = p.shape[0], 5
    rec, vis = ctx.points("hits", key, p, nrm, ids, spp, 3)
    valid = int(rec["valid"].sum())
    print(key, "points", n, "lights", ctx.table(key)["kd_ids"].shape[0], "valid share", rec["valid"].mean(),
          "visible share of the valid", vis.sum() / max(valid, 1))
    assert 0.2 < rec["valid"].mean() < 1.0 and 0.05 < vis.sum() / valid < 0.95
    want = value_of(ctx, key, rec, vis, 2)
    assert (want > 0).any()
    scene.trace_stats()
    got = direct_points(scene, p, nrm, ids, spp=spp, spp_offset=3, spp_chunk=2)
    st = scene.trace_stats()
    assert same(got, want), (key, np.argwhere(got != want)[:10])
    # the composed path: the same rays through the any-hit entry, the flags combined here
    flags, ref = occluded_flags(scene, rec)
    assert np.array_equal(rec["valid"] & ~flags, vis)
    assert same(got, value_of(ctx, key, rec, rec["valid"] & ~flags, 2))
    assert st["paths"] == spp * n and st["rays"] == st["shades"] == valid
    for k in WALK:
        assert st[k] == ref[k], (key, k, st[k], ref[k])
    _, host_ref = scene.occluded(rec["o"].reshape(-1, 3)[rec["valid"].ravel()], rec["d"].reshape(-1, 3)[rec["valid"].ravel()],
                                 rec["t_max"].ravel()[rec["valid"].ravel()])
    for k in VISITS:
        assert st[k] == host_ref[k], (key, k, st[k], host_ref[k])
    lean = direct_points(scene, p, nrm, ids, spp=spp, spp_offset=3, spp_chunk=2, lean=1)
    st = scene.trace_stats()
    assert same(lean, got)
    assert st["paths"] == spp * n and st["rays"] == st["shades"] == valid
    assert all(st[k] == 0 for k in VISITS), st
    # without the stream ids the id is the point's index; the host entry
    m = 257
    rec_i, vis_i = ctx.points("index-ids", key, p[:m], nrm[:m], np.arange(m, dtype=np.uint32), spp, 3)
    assert same(direct_points(scene, p[:m], nrm[:m], None, spp=spp, spp_offset=3, spp_chunk=2),
                value_of(ctx, key, rec_i, vis_i, 2))
    assert scene.trace_stats()["paths"] == spp * m
    host, hs = scene.direct(p, nrm, ids, spp=spp, spp_offset=3, spp_chunk=2)
    assert same(host, want)
    assert hs["paths"] == spp * n and hs["rays"] == hs["shades"] == valid
    assert scene.trace_stats()["rays"] == 0              # the host entry leaves the device entries' block alone


# ---- 2. the pixel form ---------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_pixel_form_equals_the_restatement_and_the_composed_path(ctx, key):
    import torch
    scene = ctx.scene(key)
    spp = 3
    rec, fr, vis = ctx.pixels(key, spp)
    valid, hits = int(rec["valid"].sum()), int(fr["hit"].sum())
    assert hits > W * H and 0.05 < vis.sum() / valid < 0.95
    rp = ctx.rparams(key)
    # the composed path: the primary rays through the closest-hit entry, the shadow rays through the any-hit one
    o, d = primary_rays(ctx.oracle, W, H, spp, **ctx.cam(key))
    d_o, d_d = torch.from_numpy(o.reshape(-1, 3)).cuda(), torch.from_numpy(d.reshape(-1, 3)).cuda()
    tri = torch.full((spp * W * H,), -7, dtype=torch.int32, device="cuda")
    scene.trace_stats()
    scene.trace_device(spp * W * H, d_o.data_ptr(), d_d.data_ptr(), tri.data_ptr())
    prim = scene.trace_stats()
    assert np.array_equal(tri.cpu().numpy().reshape(spp, H, W) >= 0, fr["hit"])
    flags, shadow = occluded_flags(scene, rec)
    assert np.array_equal(rec["valid"] & ~flags, vis)
    prev = (np.arange(W * H * 3, dtype=np.int64) % 17).astype(f32).reshape(H, W, 3) * f32(0.125)
    for chunk in (2, 0):
        want = value_of(ctx, key, rec, vis, chunk)
        scene.trace_stats()
        got = direct_frame(scene, rp, spp_chunk=chunk)
        st = scene.trace_stats()
        assert same(got, want), (key, chunk, np.argwhere(got != want)[:10])
        assert st["paths"] == spp * W * H and st["shades"] == valid and st["rays"] == spp * W * H + valid
        for k in VISITS:
            assert st[k] == prim[k] + shadow[k], (key, k, st[k], prim[k], shadow[k])
        assert (got[~fr["hit"].any(axis=0)] == 0).all()
        # the running mean over an earlier frame
        want2 = value_of(ctx, key, rec, vis, chunk, prev=prev, prev_count=2)
        assert same(direct_frame(scene, ctx.rparams(key, prev_count=2), prev=prev, spp_chunk=chunk), want2), chunk
        assert not same(want2, want)
    want = value_of(ctx, key, rec, vis, 2)
    scene.trace_stats()
    # scheduling, lean and the host entry: the same bits
    for kw in (dict(lean=1), dict(workgroups=2, refill=1), dict(lean=1, refill=64, workgroups=1)):
        assert same(direct_frame(scene, rp, spp_chunk=2, **kw), want), kw
    st = scene.trace_stats()
    assert st["rays"] == 3 * (spp * W * H + valid) and st["shades"] == 3 * valid
    host, hs = scene.render_direct(rp, spp_chunk=2)
    assert same(host, want) and hs["rays"] == spp * W * H + valid and hs["shades"] == valid
    host2, _ = scene.render_direct(ctx.rparams(key, prev_count=2), prev=prev, spp_chunk=2)
    assert same(host2, value_of(ctx, key, rec, vis, 2, prev=prev, prev_count=2))
    # other illum: only the factor changes
    assert same(direct_frame(scene, rp, spp_chunk=2, illum=2.5), value_of(ctx, key, rec, vis, 2, illum=2.5))


def test_pixel_form_on_a_frame_of_partial_tiles(ctx):
    key, w, h = "scene01", 37, 21
    scene = ctx.scene(key)
    rec, fr, vis = ctx.pixels(key, 4, 2, w, h)
    for tile, chunk in ((8, 3), (4, 0), (16, 1)):
        got = direct_frame(scene, ctx.rparams(key, width=w, height=h, spp=4, spp_offset=2, tile=tile), spp_chunk=chunk)
        assert same(got, value_of(ctx, key, rec, vis, chunk)), (tile, chunk)


def test_pixel_form_is_the_point_form_at_its_hits(ctx):
    key, s = "scene03", 3
    scene = ctx.scene(key)
    rec, fr, vis = ctx.pixels(key, 1, s)
    ok = fr["hit"][0]
    pix = np.nonzero(ok.ravel())[0].astype(np.uint32)
    nrm = np.where(fr["flip"][0][ok][:, None], -fr["nrm"][0][ok], fr["nrm"][0][ok]).astype(f32)
    frame = direct_frame(scene, ctx.rparams(key, spp=1, spp_offset=s))
    points = direct_points(scene, fr["hp"][0][ok], nrm, pix, spp=1, spp_offset=s)
    assert same(frame.reshape(-1, 3)[pix], points)
    assert (points > 0).any()


# ---- 3. shapes and parameters ----------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global", "scene02"])
def test_batch_shapes_chunks_and_scheduling_fields(ctx, key):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.many(key)
    spp = 5
    rec, vis = ctx.points("many", key, p, nrm, ids, spp, 5)
    contrib = R.contributions(ctx.table(key), rec, vis)
    # the chunking is part of the result: the summation orders differ somewhere
    assert not same(R.value(contrib, 0), R.value(contrib, 2))
    for n in (1, 63, 64, 65, 1025, 3000):
        got = direct_points(scene, p[:n], nrm[:n], ids[:n], spp=spp, spp_offset=5, spp_chunk=2)
        assert same(got, R.value(contrib[:, :n], 2)), (key, n)
        got = direct_points(scene, p[:n], nrm[:n], ids[:n], spp=1, spp_offset=5)
        assert same(got, R.value(contrib[:1, :n], 0)), (key, n)
    valid = int(rec["valid"].sum())
    for chunk in (0, 1, 2, spp):
        want = R.value(contrib, chunk)
        for wg in (1, 0):
            for refill in (1, 64):
                for lean in (0, 1):
                    scene.trace_stats()
                    got = direct_points(scene, p, nrm, ids, spp=spp, spp_offset=5, spp_chunk=chunk, workgroups=wg,
                                        refill=refill, lean=lean)
                    assert same(got, want), (key, chunk, wg, refill, lean)
                    st = scene.trace_stats()
                    assert st["paths"] == spp * p.shape[0] and st["rays"] == st["shades"] == valid
    # a chunk longer than the samples is one chunk; one that does not divide them
    assert same(direct_points(scene, p, nrm, ids, spp=spp, spp_offset=5, spp_chunk=64), R.value(contrib, 0))
    assert same(direct_points(scene, p, nrm, ids, spp=spp, spp_offset=5, spp_chunk=3), R.value(contrib, 3))


@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_stream_ids_a_split_and_a_shuffled_batch(ctx, key):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key, 1500)
    rec, vis = ctx.points("ids", key, p, nrm, ids, 4, 1)
    want = value_of(ctx, key, rec, vis, 2)
    whole = direct_points(scene, p, nrm, ids, spp=4, spp_offset=1, spp_chunk=2)
    assert same(whole, want)
    a = direct_points(scene, p[:700], nrm[:700], ids[:700], spp=4, spp_offset=1, spp_chunk=2)
    b = direct_points(scene, p[700:], nrm[700:], ids[700:], spp=4, spp_offset=1, spp_chunk=2)
    assert same(np.concatenate([a, b]), want)
    perm = np.random.default_rng(9).permutation(p.shape[0])
    assert same(direct_points(scene, p[perm], nrm[perm], ids[perm], spp=4, spp_offset=1, spp_chunk=2), want[perm])
    # other ids: other streams
    assert not same(direct_points(scene, p, nrm, ids + np.uint32(1), spp=4, spp_offset=1, spp_chunk=2), want)


@pytest.mark.parametrize("key", ["scene01", "scene01-global"])
def test_chained_calls_continue_the_running_mean(ctx, key):
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key, 1500)
    rec, vis = ctx.points("chain", key, p, nrm, ids, 5, 0)
    contrib = R.contributions(ctx.table(key), rec, vis)
    for chunk in (0, 2):                    # the owning lane's blend, and the finishing kernel's
        first = direct_points(scene, p, nrm, ids, spp=2, spp_offset=0, spp_chunk=chunk)
        assert same(first, R.value(contrib[:2], chunk))
        want = R.value(contrib[2:], chunk, prev=first, prev_count=1)
        got = direct_points(scene, p, nrm, ids, prev=first, spp=3, spp_offset=2, prev_count=1, spp_chunk=chunk)
        assert same(got, want), chunk
        assert not same(want, R.value(contrib[2:], chunk))
        host, _ = scene.direct(p, nrm, ids, prev=first, spp=3, spp_offset=2, prev_count=1, spp_chunk=chunk)
        assert same(host, want)


def test_bias_illum_and_seed(ctx):
    key = "scene01"
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key, 1500)
    base = direct_points(scene, p, nrm, ids, spp=3)
    for tag, kw in (("bias", dict(bias=0.25)), ("illum", dict(illum=-2.5)), ("seed", dict(seed=(1 << 40) + 12345))):
        rec, vis = ctx.points(tag, key, p, nrm, ids, 3, 0, kw.get("bias", 0.0), kw.get("seed", R.SEED))
        got = direct_points(scene, p, nrm, ids, spp=3, **kw)
        assert same(got, value_of(ctx, key, rec, vis, 0, illum=kw.get("illum", 10.0))), tag
        assert not same(got, base), tag


# ---- 4. edge cases -------------------------------------------------------------------------------

def test_points_no_light_reaches_add_exact_zeros_and_walk_nothing(ctx):
    """on scene01 by hand: a point on a face of the lamp (a box: every other face is behind the
    point's plane, its own face in it -- cx <= 0), a point between the lamp and the ceiling
    facing up (cx < 0), and a point under the lamp with a bias that swallows the distance
    (r <= 2 * bias)"""
    key = "scene01"
    scene = ctx.scene(key)
    t = ctx.table(key)
    centre = t["verts"].reshape(-1, 3).astype(np.float64).mean(axis=0)
    tri = t["verts"][0].astype(np.float64)
    on_face = tri.mean(axis=0)
    ng = t["normals"][0].astype(np.float64)
    outward = ng if np.dot(on_face - centre, ng) > 0 else -ng
    top = t["verts"][..., 1].max()
    cases = [(on_face, outward, 0.0), ((centre[0], (top + 10.0) / 2, centre[2]), (0, 1, 0), 0.0),
             ((centre[0], 5.0, centre[2]), (0, 1, 0), 20.0)]
    for x, n, bias in cases:
        p = np.tile(np.asarray(x, f32), (130, 1))
        nrm = np.tile(np.asarray(n, f32), (130, 1))
        ids = np.arange(130, dtype=np.uint32) + np.uint32(77)
        rec = R.point_samples(ctx.oracle, t, p, nrm, ids, 4, bias=bias)
        assert not rec["valid"].any(), (x, n, bias)
        for chunk in (0, 2):
            scene.trace_stats()
            got = direct_points(scene, p, nrm, ids, spp=4, spp_chunk=chunk, bias=bias)
            st = scene.trace_stats()
            assert (got.view(np.uint32) == 0).all(), (x, n, bias)
            assert st["rays"] == 0 and st["shades"] == 0 and st["paths"] == 4 * 130
            assert all(st[k] == 0 for k in VISITS)
    # the same point under the lamp with the default bias is lit
    assert (direct_points(scene, [cases[2][0]], [cases[2][1]], spp=4) > 0).all()


def test_a_model_without_emitters_writes_zeros_and_launches_no_walk(mcpt, ctx):
    m = mcpt.ObjModel(mcpt.scene_path("scene01"))
    mats = m.materials()
    assert (mats[:, 0:3] > 0).any()
    mats[:, 0:3] = 0.0
    dark = mcpt.ObjModel.from_arrays(m.vertices(), m.normals(), m.triangles(), mats, m.groups())
    scene = mcpt.Scene(dark)
    assert scene.lights()["kd_ids"].shape[0] == 0 and scene.lights()["area_total"] == 0
    p, nrm, ids = ctx.hits("scene01", 1000)
    prev = (np.arange(3000) % 13).astype(f32).reshape(1000, 3)
    rp = ctx.rparams("scene01")
    prev_px = (np.arange(W * H * 3) % 11).astype(f32).reshape(H, W, 3)
    scene.trace_stats()
    for chunk in (0, 2):
        assert (direct_points(scene, p, nrm, ids, spp=4, spp_chunk=chunk).view(np.uint32) == 0).all()
        got = direct_points(scene, p, nrm, ids, prev=prev, spp=4, spp_chunk=chunk, prev_count=2)
        assert same(got, (prev * f32(2) + f32(0)) / f32(3))
        assert (direct_frame(scene, rp, spp_chunk=chunk).view(np.uint32) == 0).all()
        got = direct_frame(scene, ctx.rparams("scene01", prev_count=2), prev=prev_px, spp_chunk=chunk)
        assert same(got, (prev_px * f32(2) + f32(0)) / f32(3))
    host, hs = scene.direct(p, nrm, ids, spp=4)
    assert (host == 0).all() and hs["rays"] == 0
    st = scene.trace_stats()
    assert st["rays"] == 0 and st["paths"] == 0 and st["shades"] == 0


# ---- 5. plumbing -------------------------------------------------------------------------------------

def test_reserve_and_no_allocation_afterwards(mcpt, ctx):
    import torch
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))      # a scene that has run no query
    p, nrm, ids = ctx.hits("scene01")
    n = p.shape[0]
    rec, vis = ctx.points("hits", "scene01", p, nrm, ids, 5, 3)
    recp, _, visp = ctx.pixels("scene01", 3)
    rp = ctx.rparams("scene01")
    d_p, d_n = torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda()
    d_s = torch.from_numpy(ids.view(np.int32)).cuda()
    out = torch.full((n, 4), SENT, dtype=torch.float32, device="cuda")
    opx = torch.full((W * H, 4), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.reserve_direct(W * H, spp=5, spp_chunk=1)                    # the most partial sums of the calls below
    free0 = scene.plan(rp)["device_free_bytes"]
    for chunk in (2, 1, 0):
        scene.direct_device(n, d_p.data_ptr(), d_n.data_ptr(), out.data_ptr(), d_s.data_ptr(), spp=5, spp_offset=3,
                            spp_chunk=chunk)
        scene.render_direct_device(rp, opx.data_ptr(), spp_chunk=chunk)
        torch.cuda.synchronize()
        assert scene.plan(rp)["device_free_bytes"] == free0
        assert same(out.cpu().numpy()[:, :3], value_of(ctx, "scene01", rec, vis, chunk))
        assert same(opx.cpu().numpy()[:, :3].reshape(H, W, 3), value_of(ctx, "scene01", recp, visp, chunk))
    assert scene.trace_stats()["paths"] == 3 * (5 * n + 3 * W * H)
    assert scene.trace_stats()["rays"] == 0                            # read and reset
    scene.direct_device(0, 0, 0, 0)                                    # n = 0 is a no-op
    assert scene.trace_stats()["rays"] == 0


def test_query_on_a_torch_stream(ctx):
    import torch
    scene = ctx.scene("scene01")
    p, nrm, ids = ctx.hits("scene01")
    rec, vis = ctx.points("hits", "scene01", p, nrm, ids, 5, 3)
    got = direct_points(scene, p, nrm, ids, stream=torch.cuda.Stream(), spp=5, spp_offset=3, spp_chunk=2)
    assert same(got, value_of(ctx, "scene01", rec, vis, 2))


def test_overlapping_buffers_are_refused_and_left_alone(mcpt, ctx):
    import torch
    scene = ctx.scene("scene01")
    n = 1024
    p, nrm, ids = ctx.hits("scene01", n)
    buf = torch.full((20 * n,), SENT, dtype=torch.float32, device="cuda")
    buf[:3 * n] = torch.from_numpy(p.ravel()).cuda()
    buf[3 * n:6 * n] = torch.from_numpy(nrm.ravel()).cuda()
    buf[6 * n:7 * n] = torch.from_numpy(ids.view(f32)).cuda()
    torch.cuda.synchronize()
    before = buf.cpu().numpy().copy()
    base = buf.data_ptr()
    P, N, S, FREE = base, base + 12 * n, base + 24 * n, base + 28 * n
    scene.trace_stats()
    for out_ptr in (P + 16, N - 16, N, S - 16, S + 4 * n - 16):
        with pytest.raises(mcpt.McptError) as e:
            scene.direct_device(n, P, N, out_ptr, S)
        assert e.value.code == -1 and "overlap" in str(e.value), out_ptr - base
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), before.view(np.uint32))
    assert scene.trace_stats()["rays"] == 0
    # adjacent, not overlapping: accepted (behind the ids, and behind that output)
    scene.direct_device(n, P, N, FREE, S, spp=3)
    scene.direct_device(n, P, N, FREE + 16 * n, 0, spp=3)
    torch.cuda.synchronize()
    rec, vis = ctx.points("sub1024", "scene01", p, nrm, ids, 3)
    rec_i, vis_i = ctx.points("sub1024-index", "scene01", p, nrm, np.arange(n, dtype=np.uint32), 3)
    got = buf.cpu().numpy()
    assert same(got[7 * n:11 * n].reshape(n, 4)[:, :3], value_of(ctx, "scene01", rec, vis))
    assert same(got[11 * n:15 * n].reshape(n, 4)[:, :3], value_of(ctx, "scene01", rec_i, vis_i))
    assert np.array_equal(got[:7 * n].view(np.uint32), before[:7 * n].view(np.uint32))
    assert (got[15 * n:] == f32(SENT)).all()


def test_trace_stats_sum_hit_ao_and_direct_queries(ctx):
    import torch
    key = "scene01"
    scene = ctx.scene(key)
    p, nrm, ids = ctx.hits(key, 1000)
    rec, vis = ctx.points("sum", key, p, nrm, ids, 2)
    valid = int(rec["valid"].sum())
    o, d = rec["o"][0], rec["d"][0]
    d_o, d_d = torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
    tri = torch.zeros((1000,), dtype=torch.int32, device="cuda")
    scene.trace_stats()
    scene.trace_device(1000, d_o.data_ptr(), d_d.data_ptr(), tri.data_ptr())
    ao_points(scene, p, nrm, ids, spp=3)
    direct_points(scene, p, nrm, ids, spp=2)
    st = scene.trace_stats()
    assert st["rays"] == 1000 + 3000 + valid
    assert st["paths"] == 3000 + 2000 and st["shades"] == 3000 + valid


def test_queries_leave_the_renders_alone(mcpt, ctx):
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), layout="global")
    keys = ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades", "renders",
            "direct_rays", "extend_rays", "clipped_rays")
    rps = (mcpt.RenderParams(width=W, height=H, spp=4, spp_chunk=2),
           mcpt.RenderParams(width=W, height=H, spp=4, pipeline="wavefront", lean=True))
    before = [scene.render(rp) for rp in rps]
    z = scene.trace_stats()                                            # after renders alone: zeros
    assert all(z[k] == 0 for k in WALK + ("paths", "shades"))
    p, nrm, ids = ctx.hits("scene01-global")
    rec, vis = ctx.points("hits", "scene01-global", p, nrm, ids, 5, 3)
    assert same(direct_points(scene, p, nrm, ids, spp=5, spp_offset=3, spp_chunk=2),
                value_of(ctx, "scene01-global", rec, vis, 2))
    recp, _, visp = ctx.pixels("scene01-global", 3)
    assert same(direct_frame(scene, ctx.rparams("scene01-global"), spp_chunk=2),
                value_of(ctx, "scene01-global", recp, visp, 2))
    for rp, (img0, st0) in zip(rps, before):                           # the queries still unread
        img1, st1 = scene.render(rp)
        assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
        for k in keys:
            assert st0[k] == st1[k], (k, st0[k], st1[k])
    st = scene.trace_stats()                                           # and the renders left the queries' alone
    assert st["paths"] == 5 * p.shape[0] + 3 * W * H


def test_two_replicas_answer_with_the_same_bits(mcpt, ctx):
    tr = mcpt.Tracer()
    try:
        tr.initialize([0, 0])
        scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
        assert scene.info()["n_devices"] == 2
        p, nrm, ids = ctx.hits("scene01")
        rec, vis = ctx.points("hits", "scene01", p, nrm, ids, 5, 3)
        assert same(direct_points(scene, p, nrm, ids, spp=5, spp_offset=3, spp_chunk=2),
                    value_of(ctx, "scene01", rec, vis, 2))
        recp, _, visp = ctx.pixels("scene01", 3)
        assert same(direct_frame(scene, ctx.rparams("scene01"), spp_chunk=2), value_of(ctx, "scene01", recp, visp, 2))
    finally:
        tr.initialize([0])
