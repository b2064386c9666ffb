"""What the radiance query tests on the GPU share (tests/test_gpu_radiance_wf.py): the
scenes of tests/test_gpu_radiance.py, its query helper with the entry as a
parameter, the kernels' summation in numpy, and the counters' rule.  Every output
tensor carries 64 guard elements behind it, checked after every query.
"""
import numpy as np

from _raysets import ray_sets
from _var_ref import chunk_lengths

f32 = np.float32
GUARD = 64
SENT = -123.5
SEED = 0x4D435054
VISITS = ("inner_visits", "leaf_visits", "leaf_refs", "tri_tests")
COUNTERS = ("rays", "paths", "shades") + VISITS
# key -> (scene, layout, eye, direction).  scene03 is a closed room: its case looks at the light from inside
CONFIGS = {
    "scene01": ("scene01", "auto", (0.0, 5.0, 17.0), (0.0, 0.0, -1.0)),
    "scene01-global": ("scene01", "global", (0.0, 5.0, 17.0), (0.0, 0.0, -1.0)),
    "scene03": ("scene03", "auto", (0.0, 5.0, 4.0), (0.0, 0.5, -1.0)),
}


class Ctx:
    """scenes, oracle scenes, ray sets and reference results, each made once"""

    def __init__(self, mcpt, oracle_mod):
        self.mcpt, self.oracle = mcpt, oracle_mod
        self._scene, self._oscene, self._rays, self._ref = {}, {}, {}, {}

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

    def unit_rays(self, key, n):
        """the same with the directions normalised in float32"""
        o, d = self.rays(key, n)
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)
        return o, np.ascontiguousarray((d / ln[:, None]).astype(f32))

    def reference(self, name, key, o, d, ids=None, **params):
        """the megakernel query's result and counters (counting), computed once per name and left alone"""
        if name not in self._ref:
            self._ref[name] = counted(self.scene(key), o, d, ids=ids, **params)
        r, st = self._ref[name]
        return r.copy(), dict(st)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def query(scene, o, d, ids=None, stream=None, prev=None, wf=None, ex=False, **params):
    """A device query on fresh torch tensors -> (n, 3) float32; the fourth component is 0 and
    the guard behind the output untouched.  wf: None -- the megakernel form, through
    Scene.radiance_device (ex: through Scene.radiance_ex_device); a dict -- the wavefront
    form with these wavefront fields.  prev: the output's old content (n, 3)"""
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
    args = (n, d_o.data_ptr(), d_d.data_ptr(), out.data_ptr(), d_s.data_ptr() if d_s is not None else 0,
            stream.cuda_stream if stream is not None else 0)
    if wf is not None:
        scene.radiance_ex_device(*args, pipeline="wavefront", **wf, **params)
    elif ex:
        scene.radiance_ex_device(*args, pipeline="megakernel", **params)
    else:
        scene.radiance_device(*args, **params)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[4 * n:] == f32(SENT)).all(), "guard behind the radiance overwritten"
    h = h[:4 * n].reshape(n, 4)
    assert (h[:, 3] == 0).all() and not np.signbit(h[:, 3]).any()
    return np.ascontiguousarray(h[:, :3])


def counted(scene, o, d, **kw):
    """query with the device entries' counters of just this call: (radiance, trace_stats)"""
    scene.trace_stats()
    r = query(scene, o, d, **kw)
    return r, scene.trace_stats()


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


def check_counters(st, ref, lean, what=None):
    """the wavefront query's rule: rays, paths and shades are the counting megakernel query's;
    the four visit counters too on a counting call, and read 0 on a lean one"""
    for k in ("rays", "paths", "shades"):
        assert st[k] == ref[k], (what, k, st[k], ref[k])
    for k in VISITS:
        assert st[k] == (0 if lean else ref[k]), (what, k, st[k], ref[k])
