"""Ambient-occlusion queries without a GPU: the C ABI's struct layout and defaults, and
every argument check that comes before a device is needed, through libmcpt.so on a
host-only scene -- for the point form (mcpt_ao_device, mcpt_ao), the pixel form
(mcpt_render_ao_device, mcpt_render_ao) and the reserve.  The checks come in the header's
order: a NULL scene, n < 0, a NULL required pointer, a field out of range (named), the
point limit and what the pixel form does not offer (MCPT_E_UNSUPPORTED), then the host-only
scene; the overlap check comes last and is reached on a device only (tests/test_gpu_ao.py).
Also a pin of the reference the GPU tests compare with (tests/_ao_ref.py): its occluded
share is a real mix, so no constant output passes them.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _ao_ref as R
from _radiance_q import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spp", "spp_offset", "radius", "bias", "seed", "prev_count", "lean", "workgroups", "refill",
         "unit_samples"]
OFFSETS = [0, 4, 8, 12, 16, 24, 28, 32, 36, 40]
SIZE = 48
DEFAULTS = dict(spp=1, spp_offset=0, radius=0.0, bias=0.0, seed=0x4D435054, prev_count=0, lean=0, workgroups=0,
                refill=0, unit_samples=0)
INVALID, UNSUPPORTED = -1, -6
TOO_MANY = (1 << 31) // 3


def _values(p):
    return {n: getattr(p, n) for n in NAMES}


def test_ao_params_default_and_layout(mcpt, tmp_path):
    from montecarlopathtracer_amd._capi import AoParamsC, RenderParamsC, lib
    p = AoParamsC(9, 9, 9.0, 9.0, 9, 9, 9, 9, 9, 9)
    lib().mcpt_ao_params_default(C.byref(p))
    assert _values(p) == DEFAULTS
    lib().mcpt_ao_params_default(None)            # no-op
    rp = RenderParamsC()
    lib().mcpt_render_params_default(C.byref(rp))
    assert p.seed == rp.seed
    assert _values(mcpt.ao_params()) == DEFAULTS
    q = mcpt.ao_params(spp=5, spp_offset=3, radius=2.5, bias=0.125, seed=(1 << 40) + 7, prev_count=4, lean=True,
                       workgroups=3, refill=64, unit_samples=2)
    assert _values(q) == dict(spp=5, spp_offset=3, radius=2.5, bias=0.125, seed=(1 << 40) + 7, prev_count=4, lean=1,
                              workgroups=3, refill=64, unit_samples=2)
    with pytest.raises(mcpt.McptError):
        mcpt.ao_params(width=3)
    assert [n for n, _ in AoParamsC._fields_] == NAMES
    assert C.sizeof(AoParamsC) == SIZE
    assert [getattr(AoParamsC, n).offset for n in NAMES] == OFFSETS
    assert lib().mcpt_abi_version() == 9
    # the header's own layout, where a C compiler is at hand
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mcpt.h"\nint main(void) {\n'
                       '  printf("%zu", sizeof(mcpt_ao_params));\n' +
                       "".join(f'  printf(" %zu", offsetof(mcpt_ao_params, {n}));\n' for n in NAMES) +
                       '  printf(" %d", MCPT_ABI_VERSION);\n'
                       '  return 0;\n}\n')
        exe = tmp_path / "layout"
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == [SIZE] + OFFSETS + [9]


# fields out of range, each with the word its message must hold
BAD_FIELDS = ((dict(spp=0), "spp"), (dict(spp=2, spp_offset=(1 << 32) - 1), "spp_offset"),
              (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"),
              (dict(bias=-0.5), "bias"), (dict(bias=float("nan")), "bias"), (dict(bias=float("inf")), "bias"),
              (dict(lean=2), "lean"), (dict(lean=-1), "lean"), (dict(workgroups=-1), "workgroups"),
              (dict(refill=-1), "refill"), (dict(refill=65), "refill"), (dict(unit_samples=-1), "unit_samples"))


def test_point_form_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    n = 8
    p = np.zeros((n, 3), np.float32)
    nr = np.tile(np.array([[0, 1, 0]], np.float32), (n, 1))
    ids = np.arange(n, dtype=np.uint32)
    out = np.zeros(n, np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    up = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    P, N, S, OUT = 1 << 20, 1 << 21, 1 << 22, 1 << 23       # never dereferenced
    vp = C.c_void_p

    def err():
        return L.mcpt_last_error().decode()

    def entries(q, n=n, scene=s.handle, p_=P, n_=N, out_=True):
        qq = C.byref(q) if q is not None else None
        return [lambda: L.mcpt_ao_device(scene, qq, n, vp(p_), vp(n_), vp(S), vp(OUT) if out_ else None, None),
                lambda: L.mcpt_ao(scene, qq, n, fp(p) if p_ else None, fp(nr) if n_ else None, up,
                                  fp(out) if out_ else None, None)]

    ok = mcpt.ao_params()
    # 1-3: a NULL scene, n < 0, a NULL required pointer with n > 0 (the stream ids may be NULL)
    for call in entries(ok, scene=None):
        assert call() == INVALID and "scene" in err()
    for call in entries(ok, n=-1):
        assert call() == INVALID and "n " in err()
    for kw in (dict(p_=0), dict(n_=0), dict(out_=False)):
        for call in entries(ok, **kw):
            assert call() == INVALID and "NULL" in err()
    # ... each before a bad field
    for call in entries(mcpt.ao_params(spp=0), scene=None):
        assert call() == INVALID and "scene" in err()
    for call in entries(mcpt.ao_params(spp=0), n=-1):
        assert call() == INVALID and "n " in err()
    for call in entries(mcpt.ao_params(spp=0), out_=False):
        assert call() == INVALID and "NULL" in err()
    # 4: fields out of range, each named -- also for an empty batch, and before the point limit
    for kw, word in BAD_FIELDS:
        for m in (n, 0, TOO_MANY):
            for call in entries(mcpt.ao_params(**kw), n=m):
                assert call() == INVALID and word in err(), (kw, m, err())
    # 5: the point limit, before the host-only scene
    for q in (ok, None):
        for call in entries(q, n=TOO_MANY):
            assert call() == UNSUPPORTED and "too many points" in err()
    # 6: otherwise valid arguments reach the host-only scene
    edge = (None, ok, mcpt.ao_params(spp=1, spp_offset=(1 << 32) - 1), mcpt.ao_params(radius=float("inf")),
            mcpt.ao_params(radius=1e-30, bias=1e-30, lean=1, workgroups=1 << 20, refill=64, unit_samples=1 << 30))
    for q in edge:
        for m in (n, 0, TOO_MANY - 1):
            for call in entries(q, n=m):
                assert call() == INVALID and "host-only" in err(), (m, err())
    # the reserve: a scene on a device, a count in range
    assert L.mcpt_scene_reserve_ao(None, 8) == INVALID and "scene" in err()
    assert L.mcpt_scene_reserve_ao(s.handle, 8) == INVALID and "not on a device" in err()
    # the Python wrappers raise the same errors
    with pytest.raises(mcpt.McptError) as e:
        s.ao(p, nr, radius=-1.0)
    assert e.value.code == INVALID and "radius" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.ao(p, nr)
    assert e.value.code == INVALID and "host-only" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.ao_device(n, P, N, OUT, unit_samples=-1)
    assert e.value.code == INVALID and "unit_samples" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.reserve_ao(8)
    assert e.value.code == INVALID


def test_pixel_form_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    W, H = 16, 8
    out = np.zeros((H, W), np.float32)
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
        return [lambda: L.mcpt_render_ao_device(scene, rr, qq, vp(OUT) if out_ else None, None),
                lambda: L.mcpt_render_ao(scene, rr, qq, fp if out_ else None, None)]

    ok = mcpt.ao_params()
    # a NULL scene, NULL render params, a NULL output: each before a bad field
    for q in (ok, mcpt.ao_params(refill=65)):
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
    # the AO params: every field is checked, the sample fields the pixel form ignores too
    for kw, word in BAD_FIELDS:
        for rp in (rparams(), rparams(mode="quinengine"), rparams(shard_count=2)):   # before what is not offered
            for call in entries(rp, mcpt.ao_params(**kw)):
                assert call() == INVALID and word in err(), (kw, err())
    # not offered: too many pixels, QuinEngine mode, shards, packed output -- before the host-only scene
    for call in entries(rparams(width=1 << 15, height=1 << 15), ok):
        assert call() == UNSUPPORTED and "too many pixels" in err()
    for call in entries(rparams(mode="quinengine"), ok):
        assert call() == UNSUPPORTED and "QuinEngine" in err()
    for kw in (dict(shard_count=2), dict(shard_count=2, shard_index=1), dict(packed=True)):
        for call in entries(rparams(**kw), ok):
            assert call() == UNSUPPORTED and "shard" in err(), kw
    # otherwise valid arguments reach the host-only scene; the render fields the query ignores are not checked
    for rp in (rparams(), rparams(tile=4), rparams(max_depth=-5), rparams(pipeline="wavefront", wf_streams=9),
               rparams(spp=1, spp_offset=(1 << 32) - 1)):
        for q in (None, ok, mcpt.ao_params(radius=3.0, lean=1, unit_samples=7)):
            for call in entries(rp, q):
                assert call() == INVALID and "host-only" in err(), err()
    with pytest.raises(mcpt.McptError) as e:
        s.render_ao(mcpt.RenderParams(width=W, height=H, spp=2), radius=-2.0)
    assert e.value.code == INVALID and "radius" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.render_ao_device(mcpt.RenderParams(width=W, height=H, spp=2), OUT)
    assert e.value.code == INVALID and "host-only" in str(e.value)


@pytest.mark.parametrize("key", ["scene01", "scene03"])
def test_the_reference_is_a_real_mix(mcpt, oracle_mod, key):
    """the restatement alone, on the frames the GPU tests use: at radii 2 and 8 between 5% and
    95% of the occlusion rays are occluded, so constant output cannot pass them"""
    name, _, eye, direction = CONFIGS[key]
    osc = oracle_mod.Scene(mcpt.scene_path(name))
    fr = R.frame(oracle_mod, osc, 64, 48, 2, eye=eye, direction=direction)
    assert fr["hit"].mean() > 0.5
    for radius in (2.0, 8.0):
        _, occ = R.pixel_reference(oracle_mod, osc, fr, radius)
        share = occ[fr["hit"]].mean()
        print(key, radius, "occluded share", share)
        assert 0.05 <= share <= 0.95, (key, radius, share)
    # the point form over the same hits with the normals turned towards the viewer (scene01's
    # shading normals mostly point away from it: unflipped, its rays leave through the walls)
    ok = fr["hit"][0]
    ids = np.nonzero(ok.ravel())[0].astype(np.uint32)
    facing = np.where(fr["flip"][0][ok][:, None], -fr["nrm"][0][ok], fr["nrm"][0][ok])
    for radius in (2.0, 8.0):
        _, occ = R.point_reference(oracle_mod, osc, fr["hp"][0][ok], facing, ids, 3, spp_offset=5, radius=radius)
        print(key, radius, "point form, facing normals: occluded share", occ.mean())
        assert 0.05 <= occ.mean() <= 0.95, (key, radius, occ.mean())
