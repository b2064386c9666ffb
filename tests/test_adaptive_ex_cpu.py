"""mcpt_render_adaptive_ex[_device] without a GPU: the symbols, their binding and
every argument check of the older pair (tests/test_adaptive_cpu.py's table),
through the general form.  The one difference: `pipeline = "wavefront"` passes
the pipeline check and reaches the host-only scene; the older pair still
refuses it.
"""
import ctypes as C

import numpy as np
import pytest


def test_ex_symbols_are_exported_and_bound(mcpt):
    from montecarlopathtracer_amd import _capi
    L = _capi.lib()
    for name in ("mcpt_render_adaptive_ex", "mcpt_render_adaptive_ex_device"):
        fn = getattr(L, name)
        old = getattr(L, name.replace("_ex", ""))
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == list(old.argtypes) and len(fn.argtypes) == 7
    assert L.mcpt_abi_version() == 9
    assert callable(mcpt.Scene.render_adaptive_ex) and callable(mcpt.Scene.render_adaptive_ex_device)


def test_render_adaptive_ex_argument_checks_without_a_device(mcpt):
    from montecarlopathtracer_amd._capi import lib
    L = lib()
    assert L.mcpt_render_adaptive_ex(None, None, None, None, None, None, None) == -1
    assert L.mcpt_render_adaptive_ex_device(None, None, None, None, None, None, None) == -1
    s = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")), host_only=True)
    fb = np.zeros((8, 8, 3), np.float32)
    var = np.zeros((8, 8, 4), np.float32)
    cnt = np.zeros((8, 8), np.uint32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    up = cnt.ctypes.data_as(C.POINTER(C.c_uint32))
    ok = mcpt.RenderParams(width=8, height=8, spp=4, spp_chunk=2)
    okc = ok.to_c()
    D = (1 << 20, 1 << 21, 1 << 22)                         # never dereferenced: every call fails first
    # NULL buffers and params
    assert L.mcpt_render_adaptive_ex(s.handle, C.byref(okc), None, None, fp(var), up, None) == -1
    assert L.mcpt_render_adaptive_ex(s.handle, C.byref(okc), None, fp(fb), None, up, None) == -1
    assert L.mcpt_render_adaptive_ex(s.handle, C.byref(okc), None, fp(fb), fp(var), None, None) == -1
    assert L.mcpt_render_adaptive_ex(s.handle, None, None, fp(fb), fp(var), up, None) == -1
    for k in range(3):
        q = [C.c_void_p(x) for x in D]
        q[k] = None
        assert L.mcpt_render_adaptive_ex_device(s.handle, C.byref(okc), None, *q, None) == -1
        assert b"NULL" in L.mcpt_last_error()
    assert L.mcpt_render_adaptive_ex_device(s.handle, None, None, *(C.c_void_p(x) for x in D), None) == -1

    def both(p, a, code, word):
        with pytest.raises(mcpt.McptError) as e:
            s.render_adaptive_ex(p, a)
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
        with pytest.raises(mcpt.McptError) as e:
            s.render_adaptive_ex_device(p, a, *D)
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))

    def table(pipeline):
        P = lambda **kw: mcpt.RenderParams(**{**dict(width=8, height=8, spp=4, spp_chunk=2,   # noqa: E731
                                                     pipeline=pipeline), **kw})
        # everything mcpt_render_var rejects
        for kw in (dict(spp_chunk=0), dict(spp_chunk=4), dict(spp=1, spp_chunk=1)):
            both(P(**kw), None, -1, "spp_chunk")
        both(P(width=0), None, -1, "width")
        both(P(max_depth=-1), None, -1, "max_depth")
        # the adaptive render's own: a running mean of its own, the sample index range
        both(P(prev_count=1), None, -1, "prev_count")
        both(P(spp_offset=2 ** 32 - 31), mcpt.adaptive_params(), -1, "spp_offset")              # 8 x 4 = 32 samples
        both(P(spp=2 ** 20, spp_chunk=2 ** 19, spp_offset=1), mcpt.adaptive_params(max_passes=4096), -1, "max_passes")
        # adaptive fields out of range, each named
        for kw, word in ((dict(max_passes=-1), "max_passes"), (dict(max_passes=4097), "max_passes"),
                         (dict(min_passes=-1), "min_passes"), (dict(max_passes=4, min_passes=5), "min_passes"),
                         (dict(min_passes=9), "min_passes"),                                       # default max 8
                         (dict(threshold=-0.5), "threshold"), (dict(threshold=float("nan")), "threshold"),
                         (dict(lum_floor=-1.0), "lum_floor"), (dict(lum_floor=float("nan")), "lum_floor"),
                         (dict(dilate=5), "dilate")):
            both(P(), mcpt.adaptive_params(**kw), -1, word)
        bad = mcpt.adaptive_params()
        bad.force_list = 2
        both(P(), bad, -1, "force_list")
        # what mcpt_render_var refuses
        for kw in (dict(shard_count=2), dict(packed=True), dict(gather="rccl")):
            both(P(**kw), None, -6, "")
        # valid arguments reach the host-only scene
        both(P(), None, -1, "host-only")
        both(P(), mcpt.adaptive_params(max_passes=4096, min_passes=4096, threshold=1e30, dilate=4, force_list=True),
             -1, "host-only")
        both(P(spp_offset=2 ** 32 - 32), None, -1, "host-only")                                   # exactly 2^32: allowed

    table("megakernel")
    table("wavefront")            # the wavefront passes the pipeline check: the same table, the same answers
    for pipeline in ("megakernel", "wavefront"):
        both(mcpt.RenderParams.for_quinengine(width=8, height=8, spp=4, spp_chunk=2, pipeline=pipeline), None, -6,
             "mode")
    # overlapping device buffers
    for ptrs in ((D[0], D[0] + 16, D[2]), (D[0], D[1], D[0] + 64), (D[0], D[1], D[1] + 1020)):
        with pytest.raises(mcpt.McptError) as e:
            s.render_adaptive_ex_device(ok, None, *ptrs)
        assert "overlap" in str(e.value)
    with pytest.raises(mcpt.McptError):
        s.render_adaptive_ex(ok, var=np.zeros((8, 8, 3), np.float32))
    # the older pair is the megakernel-only form still
    wf = mcpt.RenderParams(width=8, height=8, spp=4, spp_chunk=2, pipeline="wavefront")
    for call in (lambda: s.render_adaptive(wf), lambda: s.render_adaptive_device(wf, None, *D)):
        with pytest.raises(mcpt.McptError) as e:
            call()
        assert e.value.code == -6 and "pipeline" in str(e.value)
