"""The grid of sampler cases tests/test_gpu_math.py sends through the device samplers
(tests/hip/math_probe.hip sampler_probe) and the oracle's (orc_sample_*), and the
oracle side of that comparison.  Nothing is random: every case is a product of the
short lists below.

Normals: (0, +-1, 0); n.y = +-(1 - 2^-24) and +-(1 - 2^-22), either side of the lobe
rotation's FLT_EPSILON tests; axis-aligned; generic; generic and one ulp off unit.
Incidence: |cos| from 1 down to 2^-20 on both sides of the surface, and, for each Ni,
the critical angle and its neighbours (Ni > 1: leaving, cos^2 = 1 - 1 / Ni^2; Ni < 1:
entering, cos^2 = 1 - Ni^2 -- beyond it the reference takes the square root of a
negative number).  Uniforms: the ends of rng_next's range (2^-31, 1.0f: s = 2^31 - 1
rounds up to 1), Tr * F and its two neighbours for the Fresnel decision.
"""
import ctypes as C

import numpy as np

f32 = np.float32
U_MIN, U_BELOW_1 = f32(2.0 ** -31), f32(1 - 2.0 ** -24)
NI = [f32(v) for v in (0.5, 0.8, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 1.5, 3.0, 1000.0)]
TR = [f32(v) for v in (0.001, 0.5, 0.9, 1.0, 2.0)]
NS_U = [1, 2, 3, 50, 1000, 10 ** 6, 0xFFFFFF00]
NS_QE = [f32(v) for v in (1.5, 2.7, 10.5, 1e6)]
OPS = {"hemi": 0, "phong": 1, "phong_qe": 2, "fresnel": 3, "fresnel_qe": 4}


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum())).astype(f32)


def normals():
    out = [f32([0, 1, 0]), f32([0, -1, 0])]
    for y in (1 - 2.0 ** -24, 1 - 2.0 ** -22):
        for s in (1.0, -1.0):
            out.append(f32([np.sqrt(1 - y * y), s * y, 0.0]))
    out += [f32([1, 0, 0]), f32([-1, 0, 0]), f32([0, 0, 1]), f32([0, 0, -1])]
    generic = [_unit(v) for v in ((0.3, 0.5, -0.8), (-0.6, -0.2, 0.77), (0.1, 0.99, 0.05))]
    out += generic
    off = generic[0].copy()
    off[0] = np.nextafter(off[0], f32(2))
    out.append(off)
    off = generic[1].copy()
    off[2] = np.nextafter(off[2], f32(0))
    out.append(off)
    return out


def _tangent(n):
    a = np.array([1.0, 0.0, 0.0]) if abs(float(n[0])) < 0.9 else np.array([0.0, 1.0, 0.0])
    t = np.cross(np.asarray(n, np.float64), a)
    return t / np.sqrt((t * t).sum())


def incident(n, cos, side):
    """a unit direction with dot(in, n) ~ side * cos (side -1: arriving from outside, the entering branch)"""
    c = float(cos)
    return (side * c * np.asarray(n, np.float64) + np.sqrt(max(0.0, 1 - c * c)) * _tangent(n)).astype(f32)


def critical_cosines(ni):
    """the critical angle's cosine and its float neighbours (none for Ni == 1)"""
    ni = float(ni)
    c2 = 1 - 1 / (ni * ni) if ni > 1 else 1 - ni * ni
    if not c2 > 0:
        return []
    c = f32(np.sqrt(c2))
    return [np.nextafter(c, f32(0)), c, np.nextafter(c, f32(2))]


def tr_f(n, d, tr):
    """Tr * (1 - (1 - |dot(in, n)|)^5) in the samplers' operations (float dot, x^5 in double rounded once)"""
    ndoti = f32(f32(f32(d[0] * n[0]) + f32(d[1] * n[1])) + f32(d[2] * n[2]))
    x = np.float64(f32(f32(1) - np.abs(ndoti)))
    x2 = x * x
    return f32(f32(tr) * f32(f32(1) - f32(x2 * x2 * x)))


def lobe_cases(phong):
    """(nrm, in, u, par) arrays for the diffuse (phong None) or the Phong sampler (phong: "cv" / "qe")"""
    xs = [U_MIN, f32(0.25), f32(0.5), U_BELOW_1, f32(1.0)]
    ys = [U_MIN, f32(0.25), f32(0.7), U_BELOW_1, f32(1.0)]
    rows = []
    for n in normals():
        if phong is None:
            rows += [(n, f32([0, 0, 0]), (x, y), (0.0, 0.0)) for x in xs for y in ys]
            continue
        ins = [incident(n, 1.0, -1), incident(n, 0.6, -1), incident(n, 2.0 ** -20, 1)]
        uv = [(x, y) for x in xs[::2] for y in ys[::2]]
        if phong == "cv":
            pars = [np.array([v], np.uint32).view(f32)[0] for v in NS_U]
        else:
            pars = NS_QE
        rows += [(n, d, u, (p, 0.0)) for d in ins for u in uv for p in pars]
    return _pack(rows)


def fresnel_cases():
    ns = normals()
    rows = []
    for n in (ns[0], ns[10], ns[13]):                       # up, generic, generic one ulp off unit
        for ni in NI:
            cosines = [1.0, 0.6, 2.0 ** -20] + critical_cosines(ni)
            for c in cosines:
                for side in (-1, 1):
                    d = incident(n, c, side)
                    for tr in TR:
                        t = tr_f(n, d, tr)
                        for x in (U_MIN, f32(0.5), np.nextafter(t, f32(0)), t, np.nextafter(t, f32(4)), U_BELOW_1,
                                  f32(1.0)):
                            rows.append((n, d, (x, 0.0), (tr, ni)))
    return _pack(rows)


def _pack(rows):
    nrm = np.ascontiguousarray([r[0] for r in rows], f32)
    din = np.ascontiguousarray([r[1] for r in rows], f32)
    u = np.ascontiguousarray([r[2] for r in rows], f32)
    par = np.ascontiguousarray([r[3] for r in rows], f32)
    return nrm, din, u, par


def cases(op):
    return {"hemi": lambda: lobe_cases(None), "phong": lambda: lobe_cases("cv"), "phong_qe": lambda: lobe_cases("qe"),
            "fresnel": fresnel_cases, "fresnel_qe": fresnel_cases}[op]()


_fast = None


def _lib(oracle):
    """the oracle's samplers taking plain addresses: a loop of ctypes calls without a pointer object per argument"""
    global _fast
    if _fast is None:
        oracle.lib()
        L = C.CDLL(oracle.LIB_PATH)
        vp = C.c_void_p
        L.orc_sample_hemi.argtypes = [vp, vp, vp]
        L.orc_sample_phong.argtypes = [vp, vp, C.c_uint32, vp, vp]
        L.orc_sample_phong_qe.argtypes = [vp, vp, C.c_float, vp, vp]
        L.orc_sample_fresnel.argtypes = [vp, vp, C.c_float, C.c_float, vp, vp]
        L.orc_sample_fresnel_qe.argtypes = [vp, vp, C.c_float, C.c_float, vp, vp]
        _fast = L
    return _fast


def oracle_outputs(oracle, op, nrm, din, u, par):
    """(n, 3) float32: the oracle's sampler `op` on every case"""
    L = _lib(oracle)
    n = len(nrm)
    out = np.zeros((n, 3), f32)
    an, ad, au, ao = nrm.ctypes.data, din.ctypes.data, u.ctypes.data, out.ctypes.data
    if op == "hemi":
        for i in range(n):
            L.orc_sample_hemi(an + 12 * i, au + 8 * i, ao + 12 * i)
    elif op == "phong":
        ns = par[:, 0].copy().view(np.uint32).tolist()
        for i in range(n):
            L.orc_sample_phong(an + 12 * i, ad + 12 * i, ns[i], au + 8 * i, ao + 12 * i)
    elif op == "phong_qe":
        ns = par[:, 0].tolist()
        for i in range(n):
            L.orc_sample_phong_qe(an + 12 * i, ad + 12 * i, ns[i], au + 8 * i, ao + 12 * i)
    else:
        fn = L.orc_sample_fresnel if op == "fresnel" else L.orc_sample_fresnel_qe
        tr, ni = par[:, 0].tolist(), par[:, 1].tolist()
        for i in range(n):
            fn(an + 12 * i, ad + 12 * i, tr[i], ni[i], au + 8 * i, ao + 12 * i)
    return out
