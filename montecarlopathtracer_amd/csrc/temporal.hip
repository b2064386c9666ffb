// temporal.hip -- temporal accumulation: the temporal half of SVGF (Schied et
// al., "Spatiotemporal Variance-Guided Filtering", HPG 2017) in front of
// denoise_var.hip's spatial half.  Every pixel of the new frame finds where its
// surface was in the previous frame, fetches the accumulated colour, history
// length and variance from there if it is the same surface, and blends this
// frame in.  Needs no scene: an image-space gather over the two frames'
// feature buffers.  Per pixel (x, y), i = y W + x:
//
//   surface      cov = albedo_cov[i].w; cov <= 0: reset.  z = normal_depth[i].w / cov
//                CV: idx = (2 x / W - 1) th; idy = (hw - 2 y / W) th
//                QE: idx = (2 x / W - 1) / proj11; idy = (1 - 2 y / H) / proj22
//                w = (right idx + up idy) + fwd; d = w / |w|; o = eye (CV), eye + w (QE)
//                P = o + d z
//   reproject    v = P - eye'; zc = v . fwd'; zc <= 0: reset
//                xv = (v . right') / zc; yv = (v . up') / zc
//                CV: bx = ((xv / th' + 1) 0.5) W; by = ((hw - yv / th') 0.5) W
//                QE: bx = ((xv proj11' + 1) 0.5) W; by = ((1 - yv proj22') 0.5) H
//                l = |v|; expected depth e = l (CV), l - l / zc (QE)
//                bx, by not finite or outside [-1, W] x [-1, H]: reset
//   tap q valid  cq = hist_albedo_cov[q].w > 0, n_p . n_q >= thr (cov cq),
//                |e - zq| <= sigma_z max(e, zq) with zq = hist_normal_depth[q].w / cq
//   bilinear     the four taps around (bx, by) that are in the image, have a
//                weight > 0 and are valid: sw += w; sc += w hist_color_n[q] (N too);
//                sv += (w w) hist_var[q]
//   fallback     none: the valid pixels of the 3x3 block around the nearest
//                pixel, weight 1 each (dy outer, dx inner); still none: reset
//   blend        h = sc / sw; hv = sv / (sw sw); Ne = min(h.w, max_history - 1)
//                out = ((h Ne + c) / (Ne + 1), Ne + 1)
//                out_var = (((hv Ne) Ne + var) / ((Ne + 1) (Ne + 1)), 0)
//   reset        out = (c, 1); out_var = (var, 0)
//
// c is this frame's colour, gamma-decoded when gamma_space.  fp32, one rounding
// per operation of the list above in the written association
// (-ffp-contract=off), so tests/_temporal_ref.py restates it in numpy bit for
// bit.  A tap's loads stay behind its in-image branch and its colour and
// variance behind its validity, as in denoise_var.hip: what a rejected history
// pixel holds never reaches an output.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mcpt_device.hpp"
#include "temporal_launch.hpp"
#include "trace_device.hpp"

namespace mcpt {

using namespace dev;
using namespace trace;

namespace {

constexpr int kTpBlockX = 16, kTpBlockY = 16;   // a wave covers 16 x 4 pixels

__device__ __forceinline__ float tp_dot(float ax, float ay, float az, const float* b) {
    return (ax * b[0] + ay * b[1]) + az * b[2];
}

// the running sums of the taps that contributed
template <bool VAR>
struct TpSums {
    float4 sc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float sw = 0.0f;
    float svx = 0.0f, svy = 0.0f, svz = 0.0f;
};

// the previous frame's pixel (qx, qy) as a tap of weight wk: tested, then summed
template <bool VAR>
__device__ __forceinline__ void tp_tap(const TemporalParams& p, int qx, int qy, float wk, float4 nd, float cov, float e,
                                       const float4* __restrict__ hist_color_n, const float4* __restrict__ hist_var,
                                       const float4* __restrict__ hist_albedo_cov,
                                       const float4* __restrict__ hist_normal_depth, TpSums<VAR>& s) {
    if (qx < 0 || qy < 0 || qx >= p.width || qy >= p.height) return;
    if (!(wk > 0.0f)) return;
    const size_t q = (size_t)qy * (size_t)p.width + (size_t)qx;
    const float cq = hist_albedo_cov[q].w;
    if (!(cq > 0.0f)) return;
    const float4 nq = hist_normal_depth[q];
    const float dt = (nd.x * nq.x + nd.y * nq.y) + nd.z * nq.z;
    if (!(dt >= p.normal_threshold * (cov * cq))) return;
    const float zq = nq.w / cq;
    if (!(fabsf(e - zq) <= p.sigma_z * fmaxf(e, zq))) return;
    const float4 hc = hist_color_n[q];
    s.sw += wk;
    s.sc.x += wk * hc.x;
    s.sc.y += wk * hc.y;
    s.sc.z += wk * hc.z;
    s.sc.w += wk * hc.w;
    if constexpr (VAR) {
        const float4 hv = hist_var[q];
        const float w2 = wk * wk;
        s.svx += w2 * hv.x;
        s.svy += w2 * hv.y;
        s.svz += w2 * hv.z;
    }
}

template <bool QE, bool VAR>
__global__ void __launch_bounds__(kTpBlockX * kTpBlockY)
temporal_reproject(const TemporalParams p, const float4* __restrict__ color, const float4* __restrict__ var,
                   const float4* __restrict__ albedo_cov, const float4* __restrict__ normal_depth,
                   const float4* __restrict__ hist_color_n, const float4* __restrict__ hist_var,
                   const float4* __restrict__ hist_albedo_cov, const float4* __restrict__ hist_normal_depth,
                   float4* __restrict__ out_color_n, float4* __restrict__ out_var) {
    const int W = p.width, H = p.height;
    const int x = (int)(blockIdx.x * kTpBlockX + threadIdx.x), y = (int)(blockIdx.y * kTpBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    float4 c = color[i];
    if (p.gamma_space) {
        c.x = pow_f(c.x, kQeGamma);
        c.y = pow_f(c.y, kQeGamma);
        c.z = pow_f(c.z, kQeGamma);
    }
    float4 v4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (VAR) v4 = var[i];
    const float cov = albedo_cov[i].w;
    const float4 nd = normal_depth[i];

    TpSums<VAR> s;
    bool have = false;
    if (!(cov <= 0.0f)) {
        // this frame's surface point
        const float z = nd.w / cov;
        const float xf = (float)x, yf = (float)y;
        float idx, idy;
        if constexpr (QE) {
            idx = (2.0f * xf / p.Wf - 1.0f) / p.cur.proj11;
            idy = (1.0f - 2.0f * yf / p.Hf) / p.cur.proj22;
        } else {
            idx = (2.0f * xf / p.Wf - 1.0f) * p.cur.tan_half_fov;
            idy = (p.hw - 2.0f * yf / p.Wf) * p.cur.tan_half_fov;
        }
        const float wx = (p.cur.right[0] * idx + p.cur.up[0] * idy) + p.cur.fwd[0];
        const float wy = (p.cur.right[1] * idx + p.cur.up[1] * idy) + p.cur.fwd[1];
        const float wz = (p.cur.right[2] * idx + p.cur.up[2] * idy) + p.cur.fwd[2];
        const float len = sqrtf((wx * wx + wy * wy) + wz * wz);
        const float dx = wx / len, dy = wy / len, dz = wz / len;
        float ox = p.cur.eye[0], oy = p.cur.eye[1], oz = p.cur.eye[2];
        if constexpr (QE) {
            ox = ox + wx;
            oy = oy + wy;
            oz = oz + wz;
        }
        const float Px = ox + dx * z, Py = oy + dy * z, Pz = oz + dz * z;
        // ... in the previous camera
        const float vx = Px - p.prev.eye[0], vy = Py - p.prev.eye[1], vz = Pz - p.prev.eye[2];
        const float zc = tp_dot(vx, vy, vz, p.prev.fwd);
        if (!(zc <= 0.0f)) {
            const float xv = tp_dot(vx, vy, vz, p.prev.right) / zc;
            const float yv = tp_dot(vx, vy, vz, p.prev.up) / zc;
            float bx, by;
            if constexpr (QE) {
                bx = ((xv * p.prev.proj11 + 1.0f) * 0.5f) * p.Wf;
                by = ((1.0f - yv * p.prev.proj22) * 0.5f) * p.Hf;
            } else {
                bx = ((xv / p.prev.tan_half_fov + 1.0f) * 0.5f) * p.Wf;
                by = ((p.hw - yv / p.prev.tan_half_fov) * 0.5f) * p.Wf;
            }
            const float l = sqrtf((vx * vx + vy * vy) + vz * vz);
            float e = l;
            if constexpr (QE) e = l - l / zc;
            // (the comparisons are false for a NaN, the bounds exclude the infinities)
            if (bx >= -1.0f && bx <= p.Wf && by >= -1.0f && by <= p.Hf) {
                const float x0 = floorf(bx), y0 = floorf(by);
                const float fx = bx - x0, fy = by - y0;
                const int ix = (int)x0, iy = (int)y0;
                const float gx = 1.0f - fx, gy = 1.0f - fy;
                tp_tap<VAR>(p, ix, iy, gx * gy, nd, cov, e, hist_color_n, hist_var, hist_albedo_cov,
                            hist_normal_depth, s);
                tp_tap<VAR>(p, ix + 1, iy, fx * gy, nd, cov, e, hist_color_n, hist_var, hist_albedo_cov,
                            hist_normal_depth, s);
                tp_tap<VAR>(p, ix, iy + 1, gx * fy, nd, cov, e, hist_color_n, hist_var, hist_albedo_cov,
                            hist_normal_depth, s);
                tp_tap<VAR>(p, ix + 1, iy + 1, fx * fy, nd, cov, e, hist_color_n, hist_var, hist_albedo_cov,
                            hist_normal_depth, s);
                if (!(s.sw > 0.0f)) {
                    const int cx = (int)floorf(bx + 0.5f), cy = (int)floorf(by + 0.5f);
#pragma unroll
                    for (int ty = -1; ty <= 1; ty++)
#pragma unroll
                        for (int tx = -1; tx <= 1; tx++)
                            tp_tap<VAR>(p, cx + tx, cy + ty, 1.0f, nd, cov, e, hist_color_n, hist_var,
                                        hist_albedo_cov, hist_normal_depth, s);
                }
                have = s.sw > 0.0f;
            }
        }
    }

    float4 o = make_float4(c.x, c.y, c.z, 1.0f);
    float4 ov = make_float4(v4.x, v4.y, v4.z, 0.0f);
    if (have) {
        const float hx = s.sc.x / s.sw, hy = s.sc.y / s.sw, hz = s.sc.z / s.sw, hn = s.sc.w / s.sw;
        const float ne = fminf(hn, p.max_n);
        const float n1 = ne + 1.0f;
        o = make_float4((hx * ne + c.x) / n1, (hy * ne + c.y) / n1, (hz * ne + c.z) / n1, n1);
        if constexpr (VAR) {
            const float sw2 = s.sw * s.sw;
            const float n2 = n1 * n1;
            ov.x = ((s.svx / sw2 * ne) * ne + v4.x) / n2;
            ov.y = ((s.svy / sw2 * ne) * ne + v4.y) / n2;
            ov.z = ((s.svz / sw2 * ne) * ne + v4.z) / n2;
        }
    }
    out_color_n[i] = o;
    if constexpr (VAR) out_var[i] = ov;
}

}  // namespace

hipError_t launch_temporal(const TemporalParams& p, const float4* color, const float4* var, const float4* albedo_cov,
                           const float4* normal_depth, const float4* hist_color_n, const float4* hist_var,
                           const float4* hist_albedo_cov, const float4* hist_normal_depth, float4* out_color_n,
                           float4* out_var, hipStream_t st) {
    const dim3 block(kTpBlockX, kTpBlockY);
    const dim3 grid(((uint32_t)p.width + kTpBlockX - 1) / kTpBlockX, ((uint32_t)p.height + kTpBlockY - 1) / kTpBlockY);
    const bool qe = p.mode == kModeQE;
#define MCPT_TP_LAUNCH(QE, VAR)                                                                                  \
    hipLaunchKernelGGL((temporal_reproject<QE, VAR>), grid, block, 0, st, p, color, var, albedo_cov, normal_depth, \
                       hist_color_n, hist_var, hist_albedo_cov, hist_normal_depth, out_color_n, out_var)
    if (var) {
        if (qe) MCPT_TP_LAUNCH(true, true);
        else MCPT_TP_LAUNCH(false, true);
    } else {
        if (qe) MCPT_TP_LAUNCH(true, false);
        else MCPT_TP_LAUNCH(false, false);
    }
#undef MCPT_TP_LAUNCH
    return hipGetLastError();
}

}  // namespace mcpt
