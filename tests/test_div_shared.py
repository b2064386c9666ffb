"""The same-denominator division identity the kernel may use for the Cramer
quotients (CUTracer.cu:54-92) and normalize (Utils.hpp:27-34): for f32 a, d,
RN_f32(a * r) == a / d (IEEE) when r = RN_f64(1 / d).  Checked here with numpy on
random bit patterns, ordinary ranges, near-midpoint quotients, the IEEE
specials and the ends of the float range (edge_pairs: subnormal operands and
quotients, signed zeros, overflow) (csrc/mcpt_device.hpp recip_shared / div_shared; the device formulas
themselves are checked in tests/test_gpu_math.py)."""
import numpy as np


def edge_pairs(n=20_000, seed=19):
    """Operand pairs (a, d) at the ends of the float range, none giving NaN: subnormal
    operands on either side and on both, +-0.0 against non-zero operands, quotients that are
    subnormal or underflow to zero, quotients that overflow or end just below FLT_MAX."""
    r = np.random.default_rng(seed)
    f32 = np.float32

    def sign(c):
        return np.where(r.random(c) < 0.5, -1.0, 1.0)

    def subnormal(c):
        return (sign(c) * np.floor(2.0 ** r.uniform(0.0, 23.0, c)).clip(1, 2**23 - 1) * 2.0 ** -149).astype(f32)

    def pow2(c, lo, hi):                                    # random significands, exponents in [lo, hi)
        return (sign(c) * r.uniform(1.0, 2.0, c) * 2.0 ** r.integers(lo, hi, c)).astype(f32)

    def normal(c):
        v = r.uniform(0.5, 2.0, c)
        v[v == 0.5] = 0.75                                  # (probe op 8 divides by d - 0.5)
        return (sign(c) * v).astype(f32)
    k = n // 8
    zero = np.where(r.random(k) < 0.5, 0.0, -0.0).astype(f32)
    parts = [(subnormal(k), normal(k)),                     # subnormal quotients of subnormal numerators
             (r.uniform(-10, 10, k).astype(f32), subnormal(k)),   # overflow, or huge
             (subnormal(k), subnormal(k)),                  # ordinary quotients of two subnormals
             (pow2(k, -126, -100), pow2(k, 10, 60)),        # subnormal quotients of normal operands, underflow
             (pow2(k, 100, 128), pow2(k, -126, -10)),       # overflow and the last binades before it
             (pow2(k, 60, 128), pow2(k, -68, 0)),           # quotients around FLT_MAX
             (zero, np.concatenate([normal(k // 2), subnormal(k - k // 2)])),
             (np.concatenate([normal(k // 2), subnormal(k - k // 2)]), zero)]
    a, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    with np.errstate(all="ignore"):
        assert not np.isnan(a / d).any() and np.isfinite(a).all() and np.isfinite(d).all()
    return a, d


def shared_cases(n=1_000_000, seed=7):
    r = np.random.default_rng(seed)
    u = r.integers(0, 2**32, (2, n), dtype=np.uint64).astype(np.uint32)
    a1, b1 = u[0].view(np.float32), u[1].view(np.float32)
    a2 = r.uniform(-10, 10, n).astype(np.float32)
    b2 = r.uniform(-10, 10, n).astype(np.float32)
    # quotients next to f32 rounding midpoints: a = RN(d * m), m a 25-bit odd significand
    b3 = r.integers(1, 2**12, n).astype(np.float32)
    m = (r.integers(2**24, 2**25, n) | 1).astype(np.float64) * 2.0**-24
    a3 = (b3.astype(np.float64) * m).astype(np.float32)
    sp = np.array([0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, 1.17e-38, 1.0], np.float32)
    A, B = np.meshgrid(sp, sp)
    a4, b4 = edge_pairs()
    return (np.concatenate([a1, a2, a3, A.ravel(), a4]), np.concatenate([b1, b2, b3, B.ravel(), b4]))


def same_bits(x, y):
    return np.array_equal(x.view(np.uint32), y.view(np.uint32)) or bool(
        np.all((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))))


def test_edge_pairs_hold_the_classes_they_name():
    a, d = edge_pairs()
    tiny = np.finfo(np.float32).tiny
    with np.errstate(all="ignore"):
        q = a / d
    sub = lambda x: (np.abs(x) < tiny) & (x != 0)  # noqa: E731
    for name, count in (("subnormal a", sub(a).sum()), ("subnormal d", sub(d).sum()), ("subnormal quotient", sub(q).sum()),
                        ("underflow to zero", ((q == 0) & (a != 0)).sum()), ("overflow", (np.isinf(q) & (d != 0)).sum()),
                        ("finite above 2^120", (np.isfinite(q) & (np.abs(q) > 2.0 ** 120)).sum()),
                        ("-0.0 a", ((a == 0) & np.signbit(a)).sum()), ("+0.0 a", ((a == 0) & ~np.signbit(a)).sum()),
                        ("-0.0 d", ((d == 0) & np.signbit(d)).sum()), ("+0.0 d", ((d == 0) & ~np.signbit(d)).sum())):
        assert count >= 300, (name, int(count))


def test_shared_reciprocal_division_is_ieee():
    a, d = shared_cases()
    with np.errstate(all="ignore"):
        ref = a / d
        got = (a.astype(np.float64) * (np.float64(1) / d.astype(np.float64))).astype(np.float32)
    assert same_bits(got, ref)
