"""The radiance queries with a pipeline (mcpt_radiance_ex*) without a GPU: the
new symbols, the struct as _capi mirrors it and as the header lays it out, the
defaults, and every argument check that comes before a device is needed, through
libmcpt.so on a host-only scene.  The checks are mcpt_radiance's in its order
(tests/test_radiance_cpu.py's table, run here through the _ex entries on both
pipelines), then the wavefront fields with mcpt_render_params' ranges and
messages, then the host-only scene.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(spp=1, spp_offset=0, spp_chunk=0, max_depth=7, illum=10.0, fresnel_kd=1, seed=0x4D435054,
            prev_count=0, lean=0, workgroups=0, ready_thresh=0)
OWN = ["pipeline", "wf_batch", "wf_streams", "wf_refill", "wf_group_shift", "wf_sort", "wf_mem_limit"]
OWN_OFFSETS = [48, 52, 56, 60, 64, 68, 72]
SIZE = 80
INVALID, UNSUPPORTED = -1, -6
TOO_MANY = (1 << 31) // 3
NEW = ("mcpt_radiance_ex_params_default", "mcpt_radiance_ex_device", "mcpt_radiance_ex",
       "mcpt_scene_reserve_radiance_ex", "mcpt_scene_query_route_rays")


def test_the_new_symbols_the_struct_and_the_abi_version(mcpt, tmp_path):
    from montecarlopathtracer_amd import _capi
    for name in NEW:
        assert name in _capi.declared_symbols() and getattr(_capi.lib(), name) is not None
    assert _capi.ABI_VERSION == 9 and _capi.lib().mcpt_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "#define MCPT_ABI_VERSION 9" in hdr
    for name in NEW + ("mcpt_radiance_ex_params;",):
        assert name in hdr
    X = _capi.RadianceExParamsC
    assert [n for n, _ in X._fields_] == ["base"] + OWN
    assert C.sizeof(X) == SIZE and X.base.offset == 0 and C.sizeof(_capi.RadianceParamsC) == 48
    assert [getattr(X, n).offset for n in OWN] == OWN_OFFSETS
    for m in ("radiance_ex_device", "radiance_ex", "reserve_radiance_ex", "query_route_rays"):
        assert callable(getattr(mcpt.Scene, m))
    assert callable(mcpt.radiance_ex_params)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:                                 # the header's own layout, where a C compiler is at hand
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mcpt.h"\nint main(void) {\n'
                       '  printf("%zu %zu", sizeof(mcpt_radiance_ex_params), sizeof(mcpt_radiance_params));\n' +
                       "".join(f'  printf(" %zu", offsetof(mcpt_radiance_ex_params, {n}));\n' for n in OWN) +
                       '  return 0;\n}\n')
        exe = tmp_path / "layout"
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == [SIZE, 48] + OWN_OFFSETS


def test_defaults_are_the_megakernel_query(mcpt):
    from montecarlopathtracer_amd._capi import RadianceExParamsC, RadianceParamsC, lib
    p = RadianceExParamsC(RadianceParamsC(9, 9, 9, 9, 9.0, 9, 9, 9, 9, 9, 9), 9, 9, 9, 9, 9, 9, 9)
    lib().mcpt_radiance_ex_params_default(C.byref(p))
    b = RadianceParamsC(9, 9, 9, 9, 9.0, 9, 9, 9, 9, 9, 9)
    lib().mcpt_radiance_params_default(C.byref(b))
    assert bytes(p.base) == bytes(b)
    assert {n: getattr(p.base, n) for n in BASE} == BASE
    assert all(getattr(p, n) == 0 for n in OWN)
    lib().mcpt_radiance_ex_params_default(None)      # no-op
    q = mcpt.radiance_ex_params()
    assert bytes(q) == bytes(p)
    q = mcpt.radiance_ex_params(spp=5, illum=2.5, lean=True, pipeline="wavefront", wf_batch=1000, wf_streams=3, wf_refill=64,
                                wf_group_shift=6, wf_sort=1, wf_mem_limit=1 << 33)
    assert (q.base.spp, q.base.illum, q.base.lean) == (5, 2.5, 1)
    assert [getattr(q, n) for n in OWN] == [1, 1000, 3, 64, 6, 1, 1 << 33]
    assert mcpt.radiance_ex_params(pipeline=0).pipeline == 0 and mcpt.radiance_ex_params(pipeline="megakernel").pipeline == 0
    with pytest.raises(mcpt.McptError):
        mcpt.radiance_ex_params(width=3)


def test_argument_checks_without_a_device_on_both_pipelines(mcpt):
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

    # the old entries and the _ex entries (device, host, reserve) with the same base params and count
    def old_entries(b, n=n, scene=s.handle, o_=O, d_=D, out_=True, reserve=True):
        pp = C.byref(b) if b is not None else None
        calls = [lambda: L.mcpt_radiance_device(scene, pp, n, vp(o_), vp(d_), vp(S), vp(OUT) if out_ else None, None),
                 lambda: L.mcpt_radiance(scene, pp, n, fp(o) if o_ else None, fp(d) if d_ else None, up,
                                         fp(out) if out_ else None, None)]
        if reserve:
            calls.append(lambda: L.mcpt_scene_reserve_radiance(scene, pp, n))
        return calls

    def ex_entries(x, n=n, scene=s.handle, o_=O, d_=D, out_=True, reserve=True):
        pp = C.byref(x) if x is not None else None
        calls = [lambda: L.mcpt_radiance_ex_device(scene, pp, n, vp(o_), vp(d_), vp(S), vp(OUT) if out_ else None, None),
                 lambda: L.mcpt_radiance_ex(scene, pp, n, fp(o) if o_ else None, fp(d) if d_ else None, up,
                                            fp(out) if out_ else None, None)]
        if reserve:
            calls.append(lambda: L.mcpt_scene_reserve_radiance_ex(scene, pp, n))
        return calls

    def ex(pipeline, **kw):
        return mcpt.radiance_ex_params(pipeline=pipeline, **kw)

    # mcpt_radiance's table: the same codes and messages, in the same order, through the _ex entries
    table = []                                       # (base kwargs, call kwargs)
    ok = {}
    table += [(ok, dict(scene=None)), (ok, dict(n=-1))]
    table += [(ok, dict(reserve=False, **kw)) for kw in (dict(o_=0), dict(d_=0), dict(out_=False))]
    table += [(dict(spp=0), dict(scene=None)), (dict(spp=0), dict(n=-1)), (dict(spp=0), dict(reserve=False, out_=False))]
    bad = (dict(spp=0), dict(max_depth=-1), dict(max_depth=1001), dict(illum=float("nan")), dict(illum=float("inf")),
           dict(lean=2), dict(lean=-1), dict(fresnel_kd=2), dict(fresnel_kd=-1), dict(workgroups=-1),
           dict(ready_thresh=-1), dict(ready_thresh=65), dict(spp=2, spp_offset=(1 << 32) - 1))
    table += [(kw, dict(n=m)) for kw in bad for m in (n, 0, TOO_MANY)]
    table += [(ok, dict(n=TOO_MANY)), (dict(spp=8, spp_chunk=2), dict(n=1 << 29))]
    edge = (ok, dict(spp=1, spp_offset=(1 << 32) - 1), dict(max_depth=1000),
            dict(max_depth=0, lean=1, workgroups=1 << 20, ready_thresh=64, fresnel_kd=0, illum=0.0))
    table += [(kw, dict(n=m)) for kw in edge for m in (n, 0, TOO_MANY - 1)]
    table += [(dict(spp=8, spp_chunk=2), dict(n=(1 << 29) - 1))]
    seen = set()
    for base, kw in table:
        want = []
        for call in old_entries(mcpt.radiance_params(**base), **kw):
            want.append((call(), err()))
        assert all(c < 0 for c, _ in want)
        seen.update(c for c, _ in want)
        for pipeline in ("megakernel", "wavefront"):
            got = [(call(), err()) for call in ex_entries(ex(pipeline, **base), **kw)]
            assert got == want, (base, kw, pipeline, got, want)
    assert seen == {INVALID, UNSUPPORTED}
    # NULL params are the defaults, which select the megakernel
    for kw in (dict(), dict(n=0), dict(n=TOO_MANY)):
        want = [(call(), err()) for call in old_entries(None, **kw)]
        assert [(call(), err()) for call in ex_entries(None, **kw)] == want

    # the wavefront fields: out of range is MCPT_E_INVALID with the field named, on either pipeline, for an
    # empty batch too, behind mcpt_radiance's own checks and before the host-only scene
    wf_bad = ((dict(pipeline=2), "pipeline"), (dict(pipeline=-1), "pipeline"), (dict(wf_streams=-1), "wf_streams"),
              (dict(wf_streams=5), "wf_streams"), (dict(wf_refill=-1), "wf_refill"), (dict(wf_refill=65), "wf_refill"),
              (dict(wf_group_shift=5), "wf_group_shift"), (dict(wf_group_shift=15), "wf_group_shift"),
              (dict(wf_group_shift=-6), "wf_group_shift"))
    for kw, word in wf_bad:
        for pipeline in (0, 1):
            x = mcpt.radiance_ex_params(**{"pipeline": pipeline, **kw})
            for m in (n, 0):
                for call in ex_entries(x, n=m):
                    assert call() == INVALID and word in err(), (kw, m, err())
            for call in ex_entries(x, n=TOO_MANY):                  # the ray limit comes first
                assert call() == UNSUPPORTED and "too many rays" in err()
            x.base.spp = 0                                          # ... and so does a bad base field
            for call in ex_entries(x):
                assert call() == INVALID and "spp" in err()
    # in range: the host-only scene is what refuses
    fine = (dict(wf_streams=1), dict(wf_streams=4), dict(wf_refill=1), dict(wf_refill=64), dict(wf_group_shift=6),
            dict(wf_group_shift=14), dict(wf_sort=1), dict(wf_batch=2), dict(wf_batch=1 << 31), dict(wf_mem_limit=1))
    for kw in fine:
        for pipeline in (0, 1):
            for m in (n, 0):
                for call in ex_entries(mcpt.radiance_ex_params(pipeline=pipeline, **kw), n=m):
                    assert call() == INVALID and "host-only" in err(), (kw, err())
    # the Python mirror raises the same errors
    with pytest.raises(mcpt.McptError) as e:
        s.radiance_ex_device(n, O, D, OUT, pipeline="wavefront")
    assert e.value.code == INVALID and "host-only" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.radiance_ex_device(n, O, D, OUT, S, pipeline="wavefront", wf_streams=9)
    assert e.value.code == INVALID and "wf_streams" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.radiance_ex(o, d, stream_ids=ids, pipeline="wavefront", spp=3)
    assert e.value.code == INVALID and "host-only" in str(e.value)
    with pytest.raises(mcpt.McptError) as e:
        s.reserve_radiance_ex(n, pipeline="wavefront", wf_group_shift=3)
    assert e.value.code == INVALID and "wf_group_shift" in str(e.value)
    with pytest.raises(mcpt.McptError):
        s.radiance_ex(o, d[:3])


def test_an_empty_batch_is_a_no_op_and_a_fresh_scene_reports_no_route_rays(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    assert s.query_route_rays() == (0, 0, 0, 0)
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.mcpt_scene_query_route_rays(s.handle, out) == 0 and list(out) == [0, 0, 0, 0]
    assert L.mcpt_scene_query_route_rays(None, out) == INVALID
    assert L.mcpt_scene_query_route_rays(s.handle, None) == INVALID
    # n = 0 passes every check up to the host-only scene, which refuses (as mcpt_radiance does); on a
    # device it is a no-op (tests/test_gpu_radiance_wf.py).  The Python host entry with no rays:
    for pipeline in ("megakernel", "wavefront"):
        with pytest.raises(mcpt.McptError) as e:
            s.radiance_ex(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), pipeline=pipeline)
        assert e.value.code == INVALID and "host-only" in str(e.value)
