"""Direct-lighting queries without a GPU: the light table a scene builds at creation
(mcpt_scene_lights, host-only scenes) against the float64 restatement of
tests/_direct_ref.py, bit for bit; the selection rule; the C ABI's struct layout and
defaults; every argument check that comes before a device is needed, in the header's
order, for the point form, the pixel form and the reserve; and a radiometric pin of the
estimator itself, on the CPU alone: the restatement's area-sampling mean against a
cosine-hemisphere estimate of the same quantity through the oracle's closest hits.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _ao_ref as A
import _direct_ref as R
from _radiance_q import CONFIGS, same

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spp", "spp_offset", "spp_chunk", "illum", "bias", "seed", "prev_count", "lean", "workgroups", "refill"]
OFFSETS = [0, 4, 8, 12, 16, 24, 32, 36, 40, 44]
SIZE = 48
DEFAULTS = dict(spp=1, spp_offset=0, spp_chunk=0, illum=10.0, bias=0.0, seed=0x4D435054, prev_count=0, lean=0,
                workgroups=0, refill=0)
INVALID, UNSUPPORTED = -1, -6
TOO_MANY = (1 << 31) // 3


def _values(p):
    return {n: getattr(p, n) for n in NAMES}


# ---- the light table ---------------------------------------------------------------

@pytest.mark.parametrize("name,count", [("scene01", 12), ("scene02", 1680), ("scene03", 12)])
def test_light_table_equals_the_restatement(mcpt, oracle_mod, name, count):
    from montecarlopathtracer_amd._capi import lib
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name)), host_only=True)
    t = R.light_table(oracle_mod.Scene(mcpt.scene_path(name)))
    got = s.lights()
    assert lib().mcpt_scene_lights(s.handle, None, None, None, None) == count     # every pointer may be NULL
    assert lib().mcpt_scene_lights(None, None, None, None, None) == 0
    assert got["kd_ids"].shape[0] == count == t["kd_ids"].shape[0]
    assert np.array_equal(got["kd_ids"], t["kd_ids"])
    assert (np.diff(got["kd_ids"]) > 0).all()
    assert same(got["cdf"], t["cdf"])
    assert same(got["normals"], t["normals"])
    assert same(np.asarray([got["area_total"]]), np.asarray([t["area_total"]]))
    cdf = got["cdf"]
    assert (np.diff(cdf) >= 0).all() and cdf[-1] == f32(1.0) and cdf[0] > 0
    ln = np.sqrt((got["normals"].astype(np.float64) ** 2).sum(axis=1))
    assert np.allclose(ln, 1.0, atol=1e-6)
    assert got["area_total"] > 0


@pytest.mark.parametrize("name", ["scene01", "scene02"])
def test_selection_rule(mcpt, name):
    """u in {0, a cdf entry, the float before and after it, 1.0f}: the first entry with
    u < cdf_j, or the last -- what a binary search must return when entries are equal"""
    cdf = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path(name)), host_only=True).lights()["cdf"]
    L = cdf.shape[0]
    u = np.concatenate([[f32(0)], cdf, np.nextafter(cdf, f32(-1)), np.nextafter(cdf, f32(2)), [f32(1)]]).astype(f32)
    u = u[(u >= 0) & (u <= 1)]
    j = R.select(cdf, u)
    brute = np.minimum((cdf[None, :] <= u[:, None]).sum(axis=1), L - 1)
    assert np.array_equal(j, brute)
    assert j[0] == 0 and j[-1] == L - 1 and R.select(cdf, np.asarray([cdf[0]], f32))[0] == min(1, L - 1)
    # the kernel's search (direct.hip), restated: lo = the count of entries <= u
    for x in u[:: max(1, u.shape[0] // 200)]:
        lo, hi = 0, L
        while lo < hi:
            mid = (lo + hi) >> 1
            if cdf[mid] <= x:
                lo = mid + 1
            else:
                hi = mid
        assert min(lo, L - 1) == R.select(cdf, np.asarray([x], f32))[0]


# ---- the params ----------------------------------------------------------------------

def test_direct_params_default_and_layout(mcpt, tmp_path):
    from montecarlopathtracer_amd._capi import DirectParamsC, RenderParamsC, lib
    p = DirectParamsC(9, 9, 9, 9.0, 9.0, 9, 9, 9, 9, 9)
    lib().mcpt_direct_params_default(C.byref(p))
    assert _values(p) == DEFAULTS
    lib().mcpt_direct_params_default(None)            # no-op
    rp = RenderParamsC()
    lib().mcpt_render_params_default(C.byref(rp))
    assert p.seed == rp.seed and p.illum == rp.illum
    assert _values(mcpt.direct_params()) == DEFAULTS
    q = mcpt.direct_params(spp=5, spp_offset=3, spp_chunk=2, illum=2.5, bias=0.125, seed=(1 << 40) + 7, prev_count=4,
                           lean=True, workgroups=3, refill=64)
    assert _values(q) == dict(spp=5, spp_offset=3, spp_chunk=2, illum=2.5, bias=0.125, seed=(1 << 40) + 7,
                              prev_count=4, lean=1, workgroups=3, refill=64)
    with pytest.raises(mcpt.McptError):
        mcpt.direct_params(radius=3)
    assert [n for n, _ in DirectParamsC._fields_] == NAMES
    assert C.sizeof(DirectParamsC) == SIZE
    assert [getattr(DirectParamsC, n).offset for n in NAMES] == OFFSETS
    assert lib().mcpt_abi_version() == 9
    # the header's own layout, where a C compiler is at hand
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mcpt.h"\nint main(void) {\n'
                       '  printf("%zu", sizeof(mcpt_direct_params));\n' +
                       "".join(f'  printf(" %zu", offsetof(mcpt_direct_params, {n}));\n' for n in NAMES) +
                       '  printf(" %d", MCPT_ABI_VERSION);\n'
                       '  return 0;\n}\n')
        exe = tmp_path / "layout"
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == [SIZE] + OFFSETS + [9]


# fields out of range, each with the word its message must hold
BAD_FIELDS = ((dict(spp=0), "spp"), (dict(spp=2, spp_offset=(1 << 32) - 1), "spp_offset"),
              (dict(illum=float("nan")), "illum"), (dict(illum=float("inf")), "illum"),
              (dict(illum=float("-inf")), "illum"),
              (dict(bias=-0.5), "bias"), (dict(bias=float("nan")), "bias"), (dict(bias=float("inf")), "bias"),
              (dict(lean=2), "lean"), (dict(lean=-1), "lean"), (dict(workgroups=-1), "workgroups"),
              (dict(refill=-1), "refill"), (dict(refill=65), "refill"))


def test_point_form_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    n = 8
    p = np.zeros((n, 3), np.float32)
    nr = np.tile(np.array([[0, 1, 0]], np.float32), (n, 1))
    ids = np.arange(n, dtype=np.uint32)
    out = np.zeros((n, 3), np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    up = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    P, N, S, OUT = 1 << 20, 1 << 21, 1 << 22, 1 << 23       # never dereferenced
    vp = C.c_void_p

    def err():
        return L.mcpt_last_error().decode()

    def entries(q, n=n, scene=s.handle, p_=P, n_=N, out_=True):
        qq = C.byref(q) if q is not None else None
        return [lambda: L.mcpt_direct_device(scene, qq, n, vp(p_), vp(n_), vp(S), vp(OUT) if out_ else None, None),
                lambda: L.mcpt_direct(scene, qq, n, fp(p) if p_ else None, fp(nr) if n_ else None, up,
                                      fp(out) if out_ else None, None)]

    ok = mcpt.direct_params()
    # 1: a NULL scene, n < 0, a NULL required pointer with n > 0 (the stream ids may be NULL)
    for call in entries(ok, scene=None):
        assert call() == INVALID and "scene" in err()
    for call in entries(ok, n=-1):
        assert call() == INVALID and "n " in err()
    for kw in (dict(p_=0), dict(n_=0), dict(out_=False)):
        for call in entries(ok, **kw):
            assert call() == INVALID and "NULL" in err()
    # ... each before a bad field
    for call in entries(mcpt.direct_params(spp=0), scene=None):
        assert call() == INVALID and "scene" in err()
    for call in entries(mcpt.direct_params(spp=0), n=-1):
        assert call() == INVALID and "n " in err()
    for call in entries(mcpt.direct_params(spp=0), out_=False):
        assert call() == INVALID and "NULL" in err()
    # ... fields out of range, each named -- also for an empty batch, and before the limits
    for kw, word in BAD_FIELDS:
        for m in (n, 0, TOO_MANY):
            for call in entries(mcpt.direct_params(**kw), n=m):
                assert call() == INVALID and word in err(), (kw, m, err())
    # 2: the point limit, then the work-unit limit, before the host-only scene
    for q in (ok, None, mcpt.direct_params(spp=64, spp_chunk=1)):
        for call in entries(q, n=TOO_MANY):
            assert call() == UNSUPPORTED and "too many points" in err()
    for q, m in ((mcpt.direct_params(spp=4, spp_chunk=1), 1 << 29), (mcpt.direct_params(spp=1 << 20, spp_chunk=1), 2048),
                 (mcpt.direct_params(spp=9, spp_chunk=2), (1 << 31) // 5 + 1)):
        for call in entries(q, n=m):
            assert call() == UNSUPPORTED and "work units" in err(), err()
    # 3: otherwise valid arguments reach the host-only scene
    edge = (None, ok, mcpt.direct_params(spp=1, spp_offset=(1 << 32) - 1), mcpt.direct_params(illum=-3.0),
            mcpt.direct_params(spp=4, spp_chunk=1 << 30), mcpt.direct_params(spp=4, spp_chunk=1),
            mcpt.direct_params(bias=1e-30, illum=0.0, lean=1, workgroups=1 << 20, refill=64))
    for q in edge:
        for m in (n, 0, (1 << 29) - 1):
            for call in entries(q, n=m):
                assert call() == INVALID and "host-only" in err(), (m, err())
    # the reserve: a scene on a device, a count in range
    assert L.mcpt_scene_reserve_direct(None, None, 8) == INVALID and "scene" in err()
    assert L.mcpt_scene_reserve_direct(s.handle, None, 8) == INVALID and "not on a device" in err()
    # the Python wrappers raise the same errors
    with pytest.raises(mcpt.McptError) as e:
        s.direct(p, nr, illum=float("nan"))
    assert e.value.code == INVALID and "illum" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.direct(p, nr)
    assert e.value.code == INVALID and "host-only" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.direct_device(n, P, N, OUT, refill=70)
    assert e.value.code == INVALID and "refill" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.reserve_direct(8)
    assert e.value.code == INVALID


def test_pixel_form_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    W, H = 16, 8
    out = np.zeros((H, W, 3), np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    OUT = 1 << 23                                           # never dereferenced
    vp = C.c_void_p

    def err():
        return L.mcpt_last_error().decode()

    def rparams(**kw):
        return mcpt.RenderParams(**{**dict(width=W, height=H, spp=2), **kw}).to_c()

    def entries(rp, q, scene=s.handle, out_=True):
        rr = C.byref(rp) if rp is not None else None
        qq = C.byref(q) if q is not None else None
        return [lambda: L.mcpt_render_direct_device(scene, rr, qq, vp(OUT) if out_ else None, None),
                lambda: L.mcpt_render_direct(scene, rr, qq, fp if out_ else None, None)]

    ok = mcpt.direct_params()
    # a NULL scene, NULL render params, a NULL output: each before a bad field
    for q in (ok, mcpt.direct_params(refill=65)):
        for call in entries(rparams(), q, scene=None):
            assert call() == INVALID and "scene" in err()
        for call in entries(None, q):
            assert call() == INVALID and "params" in err()
        for call in entries(rparams(), q, out_=False):
            assert call() == INVALID and "NULL" in err()
    # the frame's fields the query reads
    for kw, word in ((dict(width=0), "width"), (dict(height=-1), "height"), (dict(spp=0), "spp"),
                     (dict(spp=2, spp_offset=(1 << 32) - 1), "spp_offset"), (dict(tile=257), "tile")):
        for call in entries(rparams(**kw), ok):
            assert call() == INVALID and word in err(), (kw, err())
    # the direct params: every field is checked, the sample fields the pixel form ignores too
    for kw, word in BAD_FIELDS:
        for rp in (rparams(), rparams(mode="quinengine"), rparams(shard_count=2)):   # before what is not offered
            for call in entries(rp, mcpt.direct_params(**kw)):
                assert call() == INVALID and word in err(), (kw, err())
    # not offered: too many pixels or work units, QuinEngine mode, shards, packed output -- before the host-only scene
    for call in entries(rparams(width=1 << 15, height=1 << 15), ok):
        assert call() == UNSUPPORTED and "too many pixels" in err()
    for call in entries(rparams(width=1 << 12, height=1 << 12, spp=256), mcpt.direct_params(spp_chunk=1)):
        assert call() == UNSUPPORTED and "work units" in err()
    for call in entries(rparams(mode="quinengine"), ok):
        assert call() == UNSUPPORTED and "QuinEngine" in err()
    for kw in (dict(shard_count=2), dict(shard_count=2, shard_index=1), dict(packed=True)):
        for call in entries(rparams(**kw), ok):
            assert call() == UNSUPPORTED and "shard" in err(), kw
    # otherwise valid arguments reach the host-only scene; the render fields the query ignores are not checked
    for rp in (rparams(), rparams(tile=4), rparams(max_depth=-5), rparams(pipeline="wavefront", wf_streams=9),
               rparams(spp=1, spp_offset=(1 << 32) - 1), rparams(width=1 << 12, height=1 << 12, spp=256)):
        for q in (None, ok, mcpt.direct_params(illum=3.0, lean=1, spp_chunk=0)):
            for call in entries(rp, q):
                assert call() == INVALID and "host-only" in err(), err()
    with pytest.raises(mcpt.McptError) as e:
        s.render_direct(mcpt.RenderParams(width=W, height=H, spp=2), illum=float("inf"))
    assert e.value.code == INVALID and "illum" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.render_direct_device(mcpt.RenderParams(width=W, height=H, spp=2), OUT)
    assert e.value.code == INVALID and "host-only" in str(e.value)


# ---- the estimator, pinned radiometrically -------------------------------------------

SPP = 4096


@pytest.mark.parametrize("key", ["scene01", "scene03"])
def test_area_sampling_agrees_with_hemisphere_sampling(mcpt, oracle_mod, key):
    """The restatement's area-sampling mean against a cosine-hemisphere estimate of the same
    quantity (E / pi): _ao_ref.point_rays -> the oracle's closest hit -> Ka * illum of the hit
    geometry if it is an emitter, else 0.  Both with SPP = 4096 samples per point, at the floor
    and wall points among the first hits of a 10 x 7 primary grid, the normals turned towards
    the viewer (not the ceiling's, whose normal points down: it sees only the lamp's top face,
    at grazing angles, where a hemisphere sample set of this size can hold no hit at all and
    then reports a standard error of 0).  Per point and channel the two means agree within 5
    combined standard errors, each computed from its own sample set; where both are zero they
    compare equal.  The lamp fills about half a percent of a hemisphere, so the hemisphere
    estimate's own error is 10-30% of the value: the pin catches a wrong constant, cosine or
    normalisation, not a small bias.  A few seconds per scene on the CPU."""
    name, _, eye, direction = CONFIGS[key]
    osc = oracle_mod.Scene(mcpt.scene_path(name))
    table = R.light_table(osc)
    fr = A.frame(oracle_mod, osc, 10, 7, 1, eye=eye, direction=direction)
    facing = np.where(fr["flip"][0][..., None], -fr["nrm"][0], fr["nrm"][0]).astype(f32)
    # floor and walls: an axis-aligned normal, not pointing down (no ceiling, no smooth-shaded object)
    ok = fr["hit"][0] & (facing[..., 1] > -0.5) & (np.abs(facing).max(axis=-1) > 0.999)
    p = np.ascontiguousarray(fr["hp"][0][ok])
    nrm = np.ascontiguousarray(facing[ok])
    ids = (np.nonzero(ok.ravel())[0] + 1000).astype(np.uint32)
    n = p.shape[0]
    assert n >= 24
    illum = 10.0
    # area sampling: the restatement itself
    _, rec, vis = R.point_reference(oracle_mod, osc, table, p, nrm, ids, SPP, illum=illum)
    a = R.contributions(table, rec, vis, illum).astype(np.float64)            # (SPP, n, 3)
    # hemisphere sampling: another stream of the same points (the seed), the oracle's closest hits
    o, d = A.point_rays(oracle_mod, p, nrm, ids, SPP, seed=A.SEED + 1)
    tri, geom, _, _ = osc.intersect(o.reshape(-1, 3), d.reshape(-1, 3), oracle_mod.KD_ORDERED, threads=8)
    g = osc.geoms()
    ka = g[np.where(tri >= 0, geom, 0), 0:3].astype(np.float64)
    emit = (tri >= 0) & (ka > 0).any(axis=1)
    h = np.where(emit[:, None], ka * illum, 0.0).reshape(SPP, n, 3)
    ma, mh = a.mean(axis=0), h.mean(axis=0)
    se = np.sqrt(a.var(axis=0, ddof=1) / SPP + h.var(axis=0, ddof=1) / SPP)
    z = np.abs(ma - mh) / np.where(se > 0, se, 1.0)
    lit = (ma > 0).any(axis=1)
    hits = emit.reshape(SPP, n).sum(axis=0)
    print(key, "hemisphere samples on the lamp per lit point: fewest", int(hits[lit].min()), "median",
          float(np.median(hits[lit])))
    print(key, "points", n, "lit", int(lit.sum()), "largest deviation in standard errors", float(z.max()),
          "mean area estimate", float(ma.mean()), "mean hemisphere estimate", float(mh.mean()))
    assert lit.sum() >= n // 2                   # a real check: most points see the light
    both_zero = (ma == 0) & (mh == 0)
    assert (np.abs(ma - mh)[~both_zero] <= 5.0 * se[~both_zero]).all(), (z.max(), np.argwhere(z > 5)[:5])
