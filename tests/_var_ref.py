"""numpy float32 restatement of the per-pixel variance (csrc/variance.hip) and of
the variance-guided a-trous denoiser (csrc/denoise_var.hip): every float
operation is one numpy float32 operation in the kernels' order, so the GPU
results are compared bit for bit.

The variance kernel reads per-chunk partial sums that no public entry returns.
They are rebuilt from plain renders: for a power-of-two chunk length n, a
CVMCTracer-mode render with spp = n, spp_offset = c n, prev_count = 0 returns
P_c / n exactly, so multiplying by n gives chunk c's partial sum bit for bit
(chunk_partials; tests/test_variance_cpu.py checks this against the oracle's
spp_chunk render).  For any other n the partial sum is the in-order float32 sum
of the chunk's n one-sample renders, which the same test checks the same way.
"""
import numpy as np

import _aov_ref as A

f32 = np.float32
LUM = (f32(0.2126), f32(0.7152), f32(0.0722))


def chunk_lengths(spp, chunk):
    return [min(chunk, spp - c) for c in range(0, spp, chunk)]


def chunk_partials(render, spp, chunk, spp_offset=0):
    """[P_c] from render(n, offset) -> the (H, W, 3) float32 mean of the n samples from
    `offset` on.  A power-of-two chunk length n: mean * n, one render.  Any other n: a
    1-spp render at offset s is sample s itself (0 + x and / 1 are exact) and the kernels
    form a chunk's sum in sample order from 0, so P_c = ((s_0 + s_1) + s_2) + ... in float32"""
    parts, off = [], spp_offset
    for n in chunk_lengths(spp, chunk):
        if n & (n - 1) == 0:
            P = (np.asarray(render(n, off), f32) * f32(n)).astype(f32)
        else:
            P = f32(0)
            for k in range(n):
                P = (P + np.asarray(render(1, off + k), f32)).astype(f32)
        parts.append(P)
        off += n
    return parts


def variance(parts, spp, chunk, prev=None, prev_count=0):
    """(mean (H, W, 3), var (H, W, 4)) from the chunk partial sums, as csrc/variance.hip"""
    ns = chunk_lengths(spp, chunk)
    K = len(ns)
    assert K == len(parts) and K >= 2
    total = np.zeros_like(parts[0])
    for P in parts:
        total = total + P
    mean = (total / f32(spp)).astype(f32)
    acc = np.zeros_like(mean)
    for P, n in zip(parts, ns):
        d = P / f32(n) - mean
        acc = acc + f32(n) * (d * d)
    var = (acc / (f32(spp) * f32(K - 1))).astype(f32)
    if prev_count > 0:
        pc, pc1 = f32(prev_count), f32(prev_count + 1)
        var = ((np.asarray(prev, f32)[..., :3] * pc) * pc + var) / (pc1 * pc1)
    out = np.zeros(var.shape[:2] + (4,), f32)
    out[..., :3] = var
    return mean, out


def _lum(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def _prefilter(a):
    """3x3 kernel 1/16 1/8 1/16, 1/8 1/4 1/8, 1/16 1/8 1/16 at unit spacing, dy outer / dx inner,
    taps outside the image skipped, divided by the sum of the weights used"""
    H, W = a.shape
    gs, gw = np.zeros((H, W), f32), np.zeros((H, W), f32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            k = f32(0.5 if dy == 0 else 0.25) * f32(0.5 if dx == 0 else 0.25)
            gs[P] = gs[P] + k * a[Q]
            gw[P] = gw[P] + k
    return (gs / gw).astype(f32)


def denoise_var(oracle, color, var, albedo_cov, normal_depth, iterations=5, normal_power_log2=7, sigma_z=0.1,
                albedo_floor=0.01, gamma_space=False, sigma_l=4.0, return_variance=False):
    """csrc/denoise_var.hip in numpy float32, the same operations in the same order;
    color (H, W, 3), var and features (H, W, 4); returns (H, W, 3) (return_variance:
    also the filtered luminance variance before the last pass drops it)"""
    col = np.asarray(color, f32)
    H, W = col.shape[:2]
    if gamma_space:
        col = A._powf(oracle, col, A.QE_GAMMA)
    alb = np.maximum(np.asarray(albedo_cov, f32)[..., :3], f32(albedo_floor))
    c = (col / alb).astype(f32)
    sd = (np.sqrt(np.maximum(np.asarray(var, f32)[..., :3], f32(0))) / alb).astype(f32)
    s = _lum(sd)
    a = (s * s).astype(f32)
    n = np.asarray(normal_depth, f32)[..., :3]
    z = np.asarray(normal_depth, f32)[..., 3]
    with np.errstate(over="ignore"):
        for i in range(iterations):
            step = 1 << i
            den = (f32(sigma_l) * np.sqrt(_prefilter(a)) + f32(1e-6)).astype(f32)
            lum = _lum(c).astype(f32)
            sc = np.zeros_like(c)
            sw = np.zeros((H, W), f32)
            sv = np.zeros((H, W), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * step, dx * step
                    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    h = A.H5[dy + 2] * A.H5[dx + 2]
                    if dy == 0 and dx == 0:
                        w = np.full((y1 - y0, x1 - x0), h, f32)
                    else:
                        np_, nq = n[P], n[Q]
                        dt = (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2]
                        wn = np.minimum(np.maximum(dt, f32(0)), f32(1))
                        for _ in range(normal_power_log2):
                            wn = wn * wn
                        r = np.abs(z[P] - z[Q]) / (f32(sigma_z) * np.maximum(z[P], z[Q]) + f32(1e-6))
                        m = np.maximum(f32(1) - r, f32(0))
                        rl = np.abs(lum[P] - lum[Q]) / den[P]
                        ml = np.maximum(f32(1) - rl, f32(0))
                        w = ((h * wn) * (m * m)) * (ml * ml)
                    sc[P] = sc[P] + w[..., None] * c[Q]
                    sw[P] = sw[P] + w
                    sv[P] = sv[P] + (w * w) * a[Q]
            c = (sc / sw[..., None]).astype(f32)
            a = (sv / (sw * sw)).astype(f32)
    out = (c * alb).astype(f32)
    if gamma_space:
        out = A._powf(oracle, out, A.QE_INV_GAMMA)
    return (out, a) if return_variance else out
