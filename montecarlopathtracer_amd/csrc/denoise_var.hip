// denoise_var.hip -- variance-guided a-trous filter: denoise.hip's edge-avoiding
// wavelet with the luminance edge-stopping weight of SVGF (Schied et al.,
// "Spatiotemporal Variance-Guided Filtering", HPG 2017), driven by the
// per-pixel variance of variance.hip and filtering that variance along with
// the colour.  Needs no scene.  The operations are denoise.hip's except:
//
//   demodulate   as denoise.hip, and the scalar luminance variance into alpha:
//                sd_c = sqrt(max(var_c, 0)) / alb_c;
//                s = (k.x sd_r + k.y sd_g) + k.z sd_b, k = (0.2126, 0.7152, 0.0722);
//                alpha = s * s   (full channel correlation: an upper bound)
//   iteration i  before the taps: g = the 3x3 kernel 1/16 1/8 1/16, 1/8 1/4 1/8,
//                1/16 1/8 1/16 over alpha at unit spacing (dy outer / dx inner,
//                taps outside the image skipped, divided by the sum of the
//                weights used); den = sigma_l * sqrt(g) + 1e-6;
//                l = (k.x c.x + k.y c.y) + k.z c.z
//                non-centre taps: rl = |lp - lq| / den; ml = max(1 - rl, 0);
//                w = ((h * wn) * wz) * (ml * ml); centre w = h
//                also sv += (w * w) * alpha_q; alpha' = sv / (sw * sw)
//   remodulate   as denoise.hip; the last pass writes alpha 0
//
// fp32, one rounding per operation of the list above (-ffp-contract=off), so
// tests/_var_ref.py restates it in numpy bit for bit.  The variance rides in
// the work buffers' alpha channel, so a tap is still two float4 loads (32 B) as
// in denoise.hip; the prefilter adds 9 dword loads per pixel and pass, which
// neighbouring lanes share.  Loads stay behind the in-image branch, as there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "aov_device.hpp"
#include "mcpt_device.hpp"
#include "trace_device.hpp"
#include "variance_launch.hpp"

namespace mcpt {

using namespace dev;
using namespace trace;
using namespace aov;

namespace {

constexpr int kDvBlockX = 16, kDvBlockY = 16;   // a wave covers 16 x 4 pixels
constexpr float kLumR = 0.2126f, kLumG = 0.7152f, kLumB = 0.0722f;

__device__ __forceinline__ V3 dv_floored_albedo(float4 a, float floor_) {
    return v3(fmaxf(a.x, floor_), fmaxf(a.y, floor_), fmaxf(a.z, floor_));
}

__device__ __forceinline__ float dv_luminance(float x, float y, float z) { return (kLumR * x + kLumG * y) + kLumB * z; }

__global__ void __launch_bounds__(kDvBlockX * kDvBlockY)
denoise_var_demodulate(const DenoiseVarParams p, const float4* __restrict__ color, const float4* __restrict__ variance,
                       const float4* __restrict__ albedo_cov, float4* __restrict__ dst) {
    const int x = (int)(blockIdx.x * kDvBlockX + threadIdx.x), y = (int)(blockIdx.y * kDvBlockY + threadIdx.y);
    if (x >= p.base.width || y >= p.base.height) return;
    const size_t i = (size_t)y * (size_t)p.base.width + (size_t)x;
    float4 c = color[i];
    if (p.base.gamma_space) {
        c.x = pow_f(c.x, kQeGamma);
        c.y = pow_f(c.y, kQeGamma);
        c.z = pow_f(c.z, kQeGamma);
    }
    const V3 alb = dv_floored_albedo(albedo_cov[i], p.base.albedo_floor);
    const float4 v = variance[i];
    const float sr = sqrtf(fmaxf(v.x, 0.0f)) / alb.x;
    const float sg = sqrtf(fmaxf(v.y, 0.0f)) / alb.y;
    const float sb = sqrtf(fmaxf(v.z, 0.0f)) / alb.z;
    const float s = dv_luminance(sr, sg, sb);
    dst[i] = make_float4(c.x / alb.x, c.y / alb.y, c.z / alb.z, s * s);
}

// one a-trous pass at `step`; LAST: remodulate (and encode) the result
template <bool LAST>
__global__ void __launch_bounds__(kDvBlockX * kDvBlockY)
denoise_var_atrous(const DenoiseVarParams p, int step, const float4* __restrict__ src,
                   const float4* __restrict__ normal_depth, const float4* __restrict__ albedo_cov,
                   float4* __restrict__ dst) {
    const int W = p.base.width, H = p.base.height;
    const int x = (int)(blockIdx.x * kDvBlockX + threadIdx.x), y = (int)(blockIdx.y * kDvBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const float4 fp = normal_depth[i];
    // 3x3 prefilter of the variance at unit spacing
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            gs += k * src[(size_t)qy * (size_t)W + (size_t)qx].w;
            gw += k;
        }
    }
    const float den = p.sigma_l * sqrtf(gs / gw) + 1e-6f;
    const float4 cp = src[i];
    const float lp = dv_luminance(cp.x, cp.y, cp.z);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
            const size_t j = (size_t)qy * (size_t)W + (size_t)qx;
            const float h = atrous_h(dy + 2) * atrous_h(dx + 2);
            float4 cq = cp;
            float w = h;
            if (dx != 0 || dy != 0) {
                cq = src[j];
                const float4 fq = normal_depth[j];
                const float dt = (fp.x * fq.x + fp.y * fq.y) + fp.z * fq.z;
                float wn = fminf(fmaxf(dt, 0.0f), 1.0f);
                for (int k = 0; k < p.base.normal_power_log2; k++) wn = wn * wn;
                const float r = fabsf(fp.w - fq.w) / (p.base.sigma_z * fmaxf(fp.w, fq.w) + 1e-6f);
                const float m = fmaxf(1.0f - r, 0.0f);
                const float wz = m * m;
                const float rl = fabsf(lp - dv_luminance(cq.x, cq.y, cq.z)) / den;
                const float ml = fmaxf(1.0f - rl, 0.0f);
                w = ((h * wn) * wz) * (ml * ml);
            }
            sx += w * cq.x;
            sy += w * cq.y;
            sz += w * cq.z;
            sw += w;
            if constexpr (!LAST) sv += (w * w) * cq.w;
        }
    }
    float ox = sx / sw, oy = sy / sw, oz = sz / sw, oa = 0.0f;
    if constexpr (LAST) {
        const V3 alb = dv_floored_albedo(albedo_cov[i], p.base.albedo_floor);
        ox = ox * alb.x;
        oy = oy * alb.y;
        oz = oz * alb.z;
        if (p.base.gamma_space) {
            ox = pow_f(ox, kQeInvGamma);
            oy = pow_f(oy, kQeInvGamma);
            oz = pow_f(oz, kQeInvGamma);
        }
    } else {
        oa = sv / (sw * sw);
    }
    dst[i] = make_float4(ox, oy, oz, oa);
}

}  // namespace

hipError_t launch_denoise_var(const DenoiseVarParams& p, const float4* color, const float4* variance,
                              const float4* albedo_cov, const float4* normal_depth, float4* out, float4* scratch,
                              hipStream_t st) {
    const dim3 block(kDvBlockX, kDvBlockY);
    const dim3 grid(((uint32_t)p.base.width + kDvBlockX - 1) / kDvBlockX,
                    ((uint32_t)p.base.height + kDvBlockY - 1) / kDvBlockY);
    const int n = p.base.iterations;
    // pass i writes out when n - 1 - i is even, so pass n - 1 lands in out; the
    // demodulated colour starts in the other buffer
    auto dst_of = [&](int i) { return ((n - 1 - i) & 1) ? scratch : out; };
    float4* cur = dst_of(0) == out ? scratch : out;
    hipLaunchKernelGGL(denoise_var_demodulate, grid, block, 0, st, p, color, variance, albedo_cov, cur);
    for (int i = 0; i < n; i++) {
        float4* dst = dst_of(i);
        if (i == n - 1)
            hipLaunchKernelGGL(denoise_var_atrous<true>, grid, block, 0, st, p, 1 << i, cur, normal_depth, albedo_cov,
                               dst);
        else
            hipLaunchKernelGGL(denoise_var_atrous<false>, grid, block, 0, st, p, 1 << i, cur, normal_depth,
                               albedo_cov, dst);
        cur = dst;
    }
    return hipGetLastError();
}

}  // namespace mcpt
