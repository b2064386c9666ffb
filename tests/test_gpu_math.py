"""Device math of the product (csrc/mcpt_device.hpp) against the CPU
specification, bit for bit: IEEE float/double division and sqrt, the fixed
sin/cos (float) and pow / x^5 (double) sequences, the TEA-16/Park-Miller RNG,
and the samplers built from them (sample_lobe_u, sample_fresnel_u) on injected
uniforms over tests/_sampler_grid.py's grid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "hip"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  (single HIP runtime)
    import build_probe
    L = C.CDLL(build_probe.build())
    fp = C.POINTER(C.c_float)
    L.math_probe.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp, C.POINTER(C.c_uint32)]

    def run(op, a, b):
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        n = a.size
        o0 = np.zeros(n, np.float32); o1 = np.zeros(n, np.float32); u = np.zeros(2 * n, np.uint32)
        rc = L.math_probe(op, n, a.ctypes.data_as(fp), b.ctypes.data_as(fp), o0.ctypes.data_as(fp),
                          o1.ctypes.data_as(fp), u.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == 0
        return o0, o1, u
    return run


@pytest.fixture(scope="module")
def sampler_probe():
    """(op name, nrm, in, u, par) -> the device sampler's (n, 3) outputs (math_probe.hip sampler_probe)"""
    import torch  # noqa: F401  (single HIP runtime)
    import build_probe
    from _sampler_grid import OPS
    L = C.CDLL(build_probe.build())
    fp = C.POINTER(C.c_float)
    L.sampler_probe.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp, fp]

    def run(op, nrm, din, u, par):
        n = len(nrm)
        assert nrm.shape == din.shape == (n, 3) and u.shape == par.shape == (n, 2)
        assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in (nrm, din, u, par))
        out = np.zeros((n, 3), np.float32)
        rc = L.sampler_probe(OPS[op], n, *(a.ctypes.data_as(fp) for a in (nrm, din, u, par, out)))
        assert rc == 0
        return out
    return run


def _inputs(n=200000, seed=0):
    r = np.random.default_rng(seed)
    a = np.concatenate([r.uniform(-10, 10, n // 2), r.standard_normal(n // 4) * 1e-3,
                        np.exp(r.uniform(-80, 80, n - n // 2 - n // 4))]).astype(np.float32)
    b = np.concatenate([r.uniform(-10, 10, n // 2), r.uniform(0.5, 2, n // 4),
                        np.exp(r.uniform(-40, 40, n - n // 2 - n // 4))]).astype(np.float32)
    # the ends of the float range: subnormal operands, +-0.0, subnormal and overflowing quotients
    from test_div_shared import edge_pairs
    ea, eb = edge_pairs()
    return np.concatenate([a, ea]), np.concatenate([b, eb])


def test_float_div_rcp_sqrt_exact(probe):
    a, b = _inputs()
    with np.errstate(all="ignore"):
        o, _, _ = probe(0, a, b)
        assert np.array_equal(o.view(np.uint32), (a / b).view(np.uint32))
        o, _, _ = probe(1, a, b)
        assert np.array_equal(o.view(np.uint32), (np.float32(1) / a).view(np.uint32))
        aa = np.abs(a)
        o, _, _ = probe(2, aa, b)
        assert np.array_equal(o.view(np.uint32), np.sqrt(aa).view(np.uint32))
        o, _, _ = probe(8, a, b)
        ref = (a - b) * (np.float32(1) / (b - np.float32(0.5)))
        assert np.array_equal(o.view(np.uint32), ref.view(np.uint32))


def test_shared_div_formulas_exact(probe):
    """ops 12 / 13: the two recip_shared variants (IEEE double 1/d; v_rcp_f64 +
    two Newton steps) give IEEE f32 a / d bit for bit (tests/test_div_shared.py)."""
    from test_div_shared import same_bits, shared_cases
    for a, d in (shared_cases(400_000, seed=11), _inputs()):     # (both end with test_div_shared.edge_pairs)
        with np.errstate(all="ignore"):
            ref = a / d
        for op in (12, 13):
            o, _, _ = probe(op, a, d)
            assert same_bits(o, ref), op


def test_double_div_exact(probe):
    a, b = _inputs()
    _, _, u = probe(5, a, b)
    got = u.view(np.uint64)
    with np.errstate(all="ignore"):
        ref = (a.astype(np.float64) / b.astype(np.float64)).view(np.uint64)
    assert np.array_equal(got, ref)


def test_sincos_pow_match_spec(probe, oracle_mod):
    L = oracle_mod.lib()
    r = np.random.default_rng(1)
    phi = (np.float32(2 * 3.14159265359) * r.random(20000, dtype=np.float32)).astype(np.float32)
    s, c, _ = probe(3, phi, phi)
    rs = np.array([L.orc_sinf(float(x)) for x in phi], np.float32)
    rc = np.array([L.orc_cosf(float(x)) for x in phi], np.float32)
    assert np.array_equal(s, rs) and np.array_equal(c, rc)
    x = r.random(20000, dtype=np.float32)
    y = (1.0 / (r.integers(1, 2000, 20000) + 1)).astype(np.float32)
    y[:5000] = 5.0
    o, _, _ = probe(4, x, y)
    ref = np.array([L.orc_powf(float(a), float(b)) for a, b in zip(x, y)], np.float32)
    assert np.array_equal(o, ref)
    o5, _, _ = probe(11, x, x)
    ref5 = np.array([L.orc_pow5f(float(a)) for a in x], np.float32)
    assert np.array_equal(o5, ref5)


def test_rng_matches_spec(probe, oracle_mod):
    L = oracle_mod.lib()
    keys = np.random.default_rng(2).integers(0, 2**32, 2000, dtype=np.uint64).astype(np.uint32)
    samples = np.arange(2000, dtype=np.uint32)
    o, _, u = probe(6, keys.view(np.float32), samples.view(np.float32))
    for i in range(0, 2000, 7):
        sd = L.orc_rng_init(i, int(keys[i]), int(samples[i]))
        assert sd == u[2 * i]
        st = C.c_uint32(sd)
        assert L.orc_rng_next(C.byref(st)) == o[i]
        assert st.value == u[2 * i + 1]


# ---- the samplers themselves, and the math at the ends of the material space ---------------

@pytest.mark.parametrize("op", ["hemi", "phong", "phong_qe", "fresnel", "fresnel_qe"])
def test_samplers_match_spec_on_the_grid(sampler_probe, oracle_mod, op):
    """sample_lobe_u (one body for diffuse and Phong, with scatter's reflection line for both
    forms of ns1) and sample_fresnel_u (one body for entering and leaving refraction, shared
    reciprocal of Ni) against the oracle's five samplers on tests/_sampler_grid.py's cases"""
    import time
    import _sampler_grid as G
    from _matzoo import same_nan_aware
    nrm, din, u, par = G.cases(op)
    t0 = time.perf_counter()
    ref = G.oracle_outputs(oracle_mod, op, nrm, din, u, par)
    dt = time.perf_counter() - t0
    got = sampler_probe(op, nrm, din, u, par)
    bad = np.flatnonzero(((got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))).any(axis=1))
    print("%s: %d cases, %d NaN outputs, oracle loop %.3f s" % (op, len(nrm), int(np.isnan(ref).any(axis=1).sum()), dt))
    assert len(bad) == 0, (op, len(bad), nrm[bad[:3]], din[bad[:3]], u[bad[:3]], par[bad[:3]], got[bad[:3]], ref[bad[:3]])
    assert same_nan_aware(got, ref)
    assert dt < 2.0


def test_pow_on_the_phong_and_gamma_domains(probe, oracle_mod):
    """op 4 where the renders call pow_f and test_sincos_pow_match_spec does not: the exponent
    1 / ns1 of every ns1 of the grid (huge, non-integer), the ends of rng_next's range, and
    the QE accumulation's x^2.2 and x^(1/2.2) over the whole float range, x > 1 included"""
    import _sampler_grid as G
    L = oracle_mod.lib()
    f32 = np.float32
    ns1 = [f32(np.uint32(v + 1)) for v in G.NS_U] + [f32(v + f32(1)) for v in G.NS_QE]
    assert ns1[len(G.NS_U) - 1] == f32(4294967040.0)
    x = np.concatenate([[G.U_MIN, G.U_BELOW_1, f32(1)], np.random.default_rng(7).random(4096, dtype=f32)]).astype(f32)
    for n1 in ns1:
        y = np.full(len(x), f32(1) / n1, f32)
        o, _, _ = probe(4, x, y)
        ref = np.array([L.orc_powf(float(a), float(y[0])) for a in x], f32)
        assert np.array_equal(o.view(np.uint32), ref.view(np.uint32)), float(n1)
    e = np.linspace(-149, 100, 4093)
    x = np.concatenate([np.exp2(e), [1.0, 2.0 ** -149, 2.0 ** 100]]).astype(f32)
    assert (x > 1).sum() > 1000 and (x == 1).any() and (x < f32(1.1754944e-38)).any() and (x > 0).all()
    for g in (f32(2.2), f32(0.454545454545)):               # trace_device.hpp kQeGamma, kQeInvGamma
        o, _, _ = probe(4, x, np.full(len(x), g, f32))
        ref = np.array([L.orc_powf(float(a), float(g)) for a in x], f32)
        assert np.array_equal(o.view(np.uint32), ref.view(np.uint32)), float(g)


def test_sincos_and_pow5_at_the_ends_of_their_arguments(probe, oracle_mod):
    """op 3 at phi = 2 * kPwPi * u for the ends of rng_next's range (u = 1.0f included: phi = 2 pi
    rounded, the reduction's k = 4); op 11 at 1 - |cos| = 0, 1 and 2^-24"""
    import _sampler_grid as G
    L = oracle_mod.lib()
    f32 = np.float32
    phi = (f32(2) * f32(3.14159265359)) * np.array([G.U_MIN, G.U_BELOW_1, f32(1)], f32)
    s, c, _ = probe(3, phi, phi)
    rs = np.array([L.orc_sinf(float(v)) for v in phi], f32)
    rc = np.array([L.orc_cosf(float(v)) for v in phi], f32)
    assert np.array_equal(s.view(np.uint32), rs.view(np.uint32)) and np.array_equal(c.view(np.uint32), rc.view(np.uint32))
    x = np.array([0.0, 1.0, 2.0 ** -24], f32)
    o, _, _ = probe(11, x, x)
    ref = np.array([L.orc_pow5f(float(v)) for v in x], f32)
    assert np.array_equal(o.view(np.uint32), ref.view(np.uint32))
    assert ref[0] == 0 and ref[1] == 1 and ref[2] == f32(2.0 ** -120)
