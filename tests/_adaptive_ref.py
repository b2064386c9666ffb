"""numpy float32 restatement of the adaptive sampler's selection, dilation,
monotone active set and per-pixel merge (csrc/adaptive.hip, DESIGN.md section
12): every float operation is one numpy float32 operation in the kernels' order.

The input is the list of per-pass (mean, var) images of the frame: pass j's
plain mean and batch-means variance (tests/_var_ref.py variance() without
prev), each over the whole image.  Because a sample's random stream depends
only on (pixel, seed, sample index), the adaptive render of a pixel that
received m passes is the uniform chain of m passes at that pixel; `adaptive`
therefore needs nothing but those images, and `uniform_chain` gives the chain
the result is compared with.  `adaptive_from_chain` takes the chain itself
(a renderer's own chained uniform calls) instead of merging per-pass images.
"""
import numpy as np

f32 = np.float32
LUM = (f32(0.2126), f32(0.7152), f32(0.0722))


def _lum(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def over(fb, var, threshold, lum_floor):
    """still noisy: the luminance of the channel standard errors against the luminance of the mean"""
    sd = np.sqrt(np.maximum(np.asarray(var, f32)[..., :3], f32(0))).astype(f32)
    s = _lum(sd)
    lum = _lum(np.asarray(fb, f32))
    with np.errstate(over="ignore"):
        return s > f32(threshold) * (lum + f32(lum_floor))


def dilate(mask, r):
    """OR over the (2r+1)^2 window, clipped to the image"""
    H, W = mask.shape
    out = np.zeros_like(mask)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            out[y0:y1, x0:x1] |= mask[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def merge(fb, var, mean, var_j, j):
    """pass j's (mean, var_j) blended into the running (fb, var) of j earlier passes"""
    if j == 0:
        return np.asarray(mean, f32).copy(), np.asarray(var_j, f32).copy()
    pc, pc1 = f32(j), f32(j + 1)
    nfb = ((fb * pc + mean) / pc1).astype(f32)
    nvar = np.zeros_like(var)
    nvar[..., :3] = ((var[..., :3] * pc) * pc + var_j[..., :3]) / (pc1 * pc1)
    return nfb, nvar


def uniform_chain(passes):
    """[(fb, var) after 1, 2, ... uniform passes]"""
    out, fb, var = [], None, None
    for j, (mean, var_j) in enumerate(passes):
        fb, var = merge(fb, var, mean, var_j, j)
        out.append((fb, var))
    return out


def adaptive_from_chain(chain, max_passes=8, min_passes=1, threshold=0.2, lum_floor=0.01, dilate_r=1):
    """`adaptive` fed with the uniform chain itself, chain[j] = (fb, var) after j + 1 uniform
    passes (a renderer's own chained calls): an active pixel of pass j takes chain[j]'s values"""
    return adaptive(chain, max_passes, min_passes, threshold, lum_floor, dilate_r, chained=True)


def adaptive(passes, max_passes=8, min_passes=1, threshold=0.2, lum_floor=0.01, dilate_r=1, chained=False):
    """(fb, var, count, active) of the adaptive render fed with the per-pass images;
    active[j] is the mask of the pixels pass j rendered (dilate_r 0: no window)"""
    mean0, var0 = passes[0]
    fb, var = merge(None, None, mean0, var0, 0)
    H, W = fb.shape[:2]
    count = np.ones((H, W), np.uint32)
    act = np.ones((H, W), bool)
    active = [act.copy()]
    for j in range(1, max_passes):
        if j < min_passes:
            act = np.ones((H, W), bool)
        else:
            prev = np.ones((H, W), bool) if (j == 1 or j == min_passes) else act
            act = prev & dilate(over(fb, var, threshold, lum_floor), dilate_r)
        if not act.any():
            break
        assert (count[act] == j).all()
        if chained:
            nfb, nvar = (np.asarray(a, f32) for a in passes[j])
        else:
            mean, var_j = passes[j]
            nfb, nvar = merge(fb, var, mean, var_j, j)
        fb = np.where(act[..., None], nfb, fb)
        var = np.where(act[..., None], nvar, var)
        count = count + act.astype(np.uint32)
        active.append(act.copy())
    return fb, var, count, active
