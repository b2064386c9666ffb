// denoise.hip -- edge-avoiding a-trous wavelet filter (Dammertz, Sewtz,
// Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global
// Illumination Filtering", HPG 2010) on albedo-demodulated colour, guided by
// the first-hit feature buffers of aov.hip.  Needs no scene.
//
//   demodulate   alb = max(albedo.rgb, floor); c = colour / alb
//                (gamma_space: colour = pow(colour, 2.2) first)
//   iteration i  step 2^i, 5x5 taps dy outer / dx inner, taps outside the image
//                skipped; h = H[dy+2] * H[dx+2], H = 1/16 1/4 3/8 1/4 1/16;
//                centre w = h; others w = (h * wn) * wz with
//                wn = clamp(np . nq, 0, 1) squared normal_power_log2 times,
//                wz = max(1 - |zp - zq| / (sigma_z * max(zp, zq) + 1e-6), 0)^2;
//                c' = sum(w c_q) / sum(w), both sums in tap order
//   remodulate   out = c * alb (gamma_space: pow(out, 1 / 2.2)), alpha 0
//
// fp32, one rounding per operation of the list above (-ffp-contract=off), so
// tests/_aov_ref.py restates it in numpy bit for bit.  One kernel per
// iteration reading its taps straight from global memory (two float4 per tap:
// the filtered colour and normal + depth; the albedo is read once per pixel);
// the passes ping-pong between out and scratch so that the last one, which also
// remodulates, lands in out.  The input colour is only read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "aov_device.hpp"
#include "aov_launch.hpp"
#include "mcpt_device.hpp"
#include "trace_device.hpp"

namespace mcpt {

using namespace dev;
using namespace trace;
using namespace aov;

namespace {

constexpr int kDnBlockX = 16, kDnBlockY = 16;   // a wave covers 16 x 4 pixels

__device__ __forceinline__ V3 floored_albedo(float4 a, float floor_) {
    return v3(fmaxf(a.x, floor_), fmaxf(a.y, floor_), fmaxf(a.z, floor_));
}

__global__ void __launch_bounds__(kDnBlockX * kDnBlockY)
denoise_demodulate(const DenoiseParams p, const float4* __restrict__ color, const float4* __restrict__ albedo_cov,
                   float4* __restrict__ dst) {
    const int x = (int)(blockIdx.x * kDnBlockX + threadIdx.x), y = (int)(blockIdx.y * kDnBlockY + threadIdx.y);
    if (x >= p.width || y >= p.height) return;
    const size_t i = (size_t)y * (size_t)p.width + (size_t)x;
    float4 c = color[i];
    if (p.gamma_space) {
        c.x = pow_f(c.x, kQeGamma);
        c.y = pow_f(c.y, kQeGamma);
        c.z = pow_f(c.z, kQeGamma);
    }
    const V3 alb = floored_albedo(albedo_cov[i], p.albedo_floor);
    dst[i] = make_float4(c.x / alb.x, c.y / alb.y, c.z / alb.z, 0.0f);
}

// one a-trous pass at `step`; LAST: remodulate (and encode) the result
template <bool LAST>
__global__ void __launch_bounds__(kDnBlockX * kDnBlockY)
denoise_atrous(const DenoiseParams p, int step, const float4* __restrict__ src, const float4* __restrict__ normal_depth,
               const float4* __restrict__ albedo_cov, float4* __restrict__ dst) {
    const int x = (int)(blockIdx.x * kDnBlockX + threadIdx.x), y = (int)(blockIdx.y * kDnBlockY + threadIdx.y);
    if (x >= p.width || y >= p.height) return;
    const size_t i = (size_t)y * (size_t)p.width + (size_t)x;
    const float4 fp = normal_depth[i];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qy < 0 || qx >= p.width || qy >= p.height) continue;
            const size_t j = (size_t)qy * (size_t)p.width + (size_t)qx;
            const float4 cq = src[j];
            const float h = atrous_h(dy + 2) * atrous_h(dx + 2);
            float w = h;
            if (dx != 0 || dy != 0) {
                const float4 fq = normal_depth[j];
                const float dt = (fp.x * fq.x + fp.y * fq.y) + fp.z * fq.z;
                float wn = fminf(fmaxf(dt, 0.0f), 1.0f);
                for (int k = 0; k < p.normal_power_log2; k++) wn = wn * wn;
                const float r = fabsf(fp.w - fq.w) / (p.sigma_z * fmaxf(fp.w, fq.w) + 1e-6f);
                const float m = fmaxf(1.0f - r, 0.0f);
                const float wz = m * m;
                w = (h * wn) * wz;
            }
            sx += w * cq.x;
            sy += w * cq.y;
            sz += w * cq.z;
            sw += w;
        }
    }
    float ox = sx / sw, oy = sy / sw, oz = sz / sw;
    if constexpr (LAST) {
        const V3 alb = floored_albedo(albedo_cov[i], p.albedo_floor);
        ox = ox * alb.x;
        oy = oy * alb.y;
        oz = oz * alb.z;
        if (p.gamma_space) {
            ox = pow_f(ox, kQeInvGamma);
            oy = pow_f(oy, kQeInvGamma);
            oz = pow_f(oz, kQeInvGamma);
        }
    }
    dst[i] = make_float4(ox, oy, oz, 0.0f);
}

}  // namespace

hipError_t launch_denoise(const DenoiseParams& p, const float4* color, const float4* albedo_cov,
                          const float4* normal_depth, float4* out, float4* scratch, hipStream_t st) {
    const dim3 block(kDnBlockX, kDnBlockY);
    const dim3 grid(((uint32_t)p.width + kDnBlockX - 1) / kDnBlockX, ((uint32_t)p.height + kDnBlockY - 1) / kDnBlockY);
    const int n = p.iterations;
    // pass i writes out when n - 1 - i is even, so pass n - 1 lands in out; the
    // demodulated colour starts in the other buffer
    auto dst_of = [&](int i) { return ((n - 1 - i) & 1) ? scratch : out; };
    float4* cur = dst_of(0) == out ? scratch : out;
    hipLaunchKernelGGL(denoise_demodulate, grid, block, 0, st, p, color, albedo_cov, cur);
    for (int i = 0; i < n; i++) {
        float4* dst = dst_of(i);
        if (i == n - 1)
            hipLaunchKernelGGL(denoise_atrous<true>, grid, block, 0, st, p, 1 << i, cur, normal_depth, albedo_cov, dst);
        else
            hipLaunchKernelGGL(denoise_atrous<false>, grid, block, 0, st, p, 1 << i, cur, normal_depth, albedo_cov, dst);
        cur = dst;
    }
    return hipGetLastError();
}

}  // namespace mcpt
