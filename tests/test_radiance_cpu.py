"""Device radiance queries without a GPU: the C ABI's struct layout and
defaults, and every argument check that comes before a device is needed, through
libmcpt.so on a host-only scene -- for the two query entries
(mcpt_radiance_device, mcpt_radiance) and the reserve.  The checks come in the
header's order: a NULL scene, n < 0, a NULL required pointer, a field out of
range (named), the ray / work-unit limits (MCPT_E_UNSUPPORTED), then the
host-only scene; the overlap check comes last and is reached on a device only
(tests/test_gpu_radiance.py).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spp", "spp_offset", "spp_chunk", "max_depth", "illum", "fresnel_kd", "seed", "prev_count", "lean",
         "workgroups", "ready_thresh"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 32, 36, 40, 44]
SIZE = 48
DEFAULTS = dict(spp=1, spp_offset=0, spp_chunk=0, max_depth=7, illum=10.0, fresnel_kd=1, seed=0x4D435054,
                prev_count=0, lean=0, workgroups=0, ready_thresh=0)
INVALID, UNSUPPORTED = -1, -6
TOO_MANY = (1 << 31) // 3


def _values(p):
    return {n: getattr(p, n) for n in NAMES}


def test_radiance_params_default_and_layout(mcpt, tmp_path):
    from montecarlopathtracer_amd._capi import RadianceParamsC, RenderParamsC, lib
    p = RadianceParamsC(9, 9, 9, 9, 9.0, 9, 9, 9, 9, 9, 9)
    lib().mcpt_radiance_params_default(C.byref(p))
    assert _values(p) == DEFAULTS
    lib().mcpt_radiance_params_default(None)      # no-op
    rp = RenderParamsC()
    lib().mcpt_render_params_default(C.byref(rp))
    assert p.seed == rp.seed and p.max_depth == rp.max_depth and p.illum == rp.illum and p.fresnel_kd == rp.fresnel_kd
    assert _values(mcpt.radiance_params()) == DEFAULTS
    q = mcpt.radiance_params(spp=5, spp_offset=3, spp_chunk=2, max_depth=0, illum=2.5, fresnel_kd=0, seed=(1 << 40) + 7,
                             prev_count=4, lean=True, workgroups=3, ready_thresh=64)
    assert _values(q) == dict(spp=5, spp_offset=3, spp_chunk=2, max_depth=0, illum=2.5, fresnel_kd=0,
                              seed=(1 << 40) + 7, prev_count=4, lean=1, workgroups=3, ready_thresh=64)
    with pytest.raises(mcpt.McptError):
        mcpt.radiance_params(width=3)
    assert [n for n, _ in RadianceParamsC._fields_] == NAMES
    assert C.sizeof(RadianceParamsC) == SIZE
    assert [getattr(RadianceParamsC, n).offset for n in NAMES] == OFFSETS
    assert lib().mcpt_abi_version() == 9
    # the header's own layout, where a C compiler is at hand
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mcpt.h"\nint main(void) {\n'
                       '  printf("%zu", sizeof(mcpt_radiance_params));\n' +
                       "".join(f'  printf(" %zu", offsetof(mcpt_radiance_params, {n}));\n' for n in NAMES) +
                       '  printf(" %d", MCPT_ABI_VERSION);\n'
                       '  return 0;\n}\n')
        exe = tmp_path / "layout"
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == [SIZE] + OFFSETS + [9]


def test_radiance_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    n = 8
    o = np.zeros((n, 3), np.float32)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (n, 1))
    ids = np.arange(n, dtype=np.uint32)
    out = np.zeros((n, 3), np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    up = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    O, D, S, OUT = 1 << 20, 1 << 21, 1 << 22, 1 << 23       # never dereferenced
    vp = C.c_void_p

    def err():
        return L.mcpt_last_error().decode()

    # the device entry, the host entry and the reserve (which takes no pointers) with the same params and count
    def entries(p, n=n, scene=s.handle, o_=O, d_=D, out_=True, reserve=True):
        pp = C.byref(p) if p is not None else None
        calls = [lambda: L.mcpt_radiance_device(scene, pp, n, vp(o_), vp(d_), vp(S), vp(OUT) if out_ else None, None),
                 lambda: L.mcpt_radiance(scene, pp, n, fp(o) if o_ else None, fp(d) if d_ else None, up,
                                         fp(out) if out_ else None, None)]
        if reserve:
            calls.append(lambda: L.mcpt_scene_reserve_radiance(scene, pp, n))
        return calls

    ok = mcpt.radiance_params()
    # 1-3: a NULL scene, n < 0, a NULL required pointer with n > 0 (the stream ids may be NULL)
    for call in entries(ok, scene=None):
        assert call() == INVALID and "scene" in err()
    for call in entries(ok, n=-1):
        assert call() == INVALID and "n " in err()
    for kw in (dict(o_=0), dict(d_=0), dict(out_=False)):
        for call in entries(ok, reserve=False, **kw):
            assert call() == INVALID and "NULL" in err()
    # ... each before a bad field
    for call in entries(mcpt.radiance_params(spp=0), scene=None):
        assert call() == INVALID and "scene" in err()
    for call in entries(mcpt.radiance_params(spp=0), n=-1):
        assert call() == INVALID and "n " in err()
    for call in entries(mcpt.radiance_params(spp=0), reserve=False, out_=False):
        assert call() == INVALID and "NULL" in err()
    # 4: fields out of range, each named
    bad = ((dict(spp=0), "spp"), (dict(max_depth=-1), "max_depth"), (dict(max_depth=1001), "max_depth"),
           (dict(illum=float("nan")), "illum"), (dict(illum=float("inf")), "illum"), (dict(lean=2), "lean"),
           (dict(lean=-1), "lean"), (dict(fresnel_kd=2), "fresnel_kd"), (dict(fresnel_kd=-1), "fresnel_kd"),
           (dict(workgroups=-1), "workgroups"), (dict(ready_thresh=-1), "ready_thresh"),
           (dict(ready_thresh=65), "ready_thresh"), (dict(spp=2, spp_offset=(1 << 32) - 1), "spp_offset"))
    for kw, word in bad:
        for m in (n, 0, TOO_MANY):              # also for an empty batch, and before the ray limit
            for call in entries(mcpt.radiance_params(**kw), n=m):
                assert call() == INVALID and word in err(), (kw, m, err())
    # 5: the ray limit and the unit limit, before the host-only scene
    for p in (ok, None):
        for call in entries(p, n=TOO_MANY):
            assert call() == UNSUPPORTED and "too many rays" in err()
    many = mcpt.radiance_params(spp=8, spp_chunk=2)             # four chunks
    for call in entries(many, n=1 << 29):
        assert call() == UNSUPPORTED and "work units" in err()
    # 6: otherwise valid arguments reach the host-only scene
    edge = (None, ok, mcpt.radiance_params(spp=1, spp_offset=(1 << 32) - 1), mcpt.radiance_params(max_depth=1000),
            mcpt.radiance_params(max_depth=0, lean=1, workgroups=1 << 20, ready_thresh=64, fresnel_kd=0, illum=0.0))
    for p in edge:
        for m in (n, 0, TOO_MANY - 1):
            for call in entries(p, n=m):
                assert call() == INVALID and "host-only" in err(), (m, err())
    for call in entries(many, n=(1 << 29) - 1):
        assert call() == INVALID and "host-only" in err()
    # the Python mirror raises the same errors
    with pytest.raises(mcpt.McptError) as e:
        s.radiance_device(n, O, D, OUT)
    assert e.value.code == INVALID and "host-only" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.radiance_device(n, O, D, OUT, S, ready_thresh=99)
    assert e.value.code == INVALID and "ready_thresh" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.radiance_device(TOO_MANY, O, D, OUT)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(mcpt.McptError) as e:
        s.radiance(o, d, stream_ids=ids, spp=3)
    assert e.value.code == INVALID and "host-only" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.radiance(o, d, spp=0)
    assert e.value.code == INVALID and "spp" in str(e.value)
    with pytest.raises(mcpt.McptError):
        s.radiance(o, d, stream_ids=ids[:3])
    with pytest.raises(mcpt.McptError):
        s.radiance(o, d[:3])
    with pytest.raises(mcpt.McptError) as e:
        s.reserve_radiance(n, spp=4)
    assert e.value.code == INVALID and "host-only" in str(e.value)


def test_every_radiance_entry_is_declared_and_the_abi_version_stays(mcpt):
    from montecarlopathtracer_amd import _capi
    for name in ("mcpt_radiance_params_default", "mcpt_radiance_device", "mcpt_radiance",
                 "mcpt_scene_reserve_radiance"):
        assert name in _capi.declared_symbols() and getattr(_capi.lib(), name) is not None
    assert _capi.ABI_VERSION == 9 and _capi.lib().mcpt_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "#define MCPT_ABI_VERSION 9" in hdr
    for name in ("mcpt_radiance_params_default", "mcpt_radiance_device", "mcpt_radiance",
                 "mcpt_scene_reserve_radiance", "mcpt_radiance_params;"):
        assert name in hdr
    for m in ("radiance_device", "radiance", "reserve_radiance"):
        assert callable(getattr(mcpt.Scene, m))
    assert callable(mcpt.radiance_params)
