// aov_device.hpp -- device helpers of the first-hit feature buffers (aov.hip)
// and the a-trous denoiser (denoise.hip).  fp32 only, one operation per
// statement of the specification, so both are
// restatable in numpy bit for bit (tests/_aov_ref.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcpt_device.hpp"
#include "render_launch.hpp"
#include "trace_device.hpp"

namespace mcpt {
namespace aov {

using namespace dev;
using namespace trace;

// the factor the first scatter at a hit on g multiplies into the throughput
// (scatter_n: CUTracer.cu:128-160; emitters end the path with no factor)
__device__ __forceinline__ V3 first_scatter_albedo(const GpuGeom& g, int32_t fresnel_kd) {
    if (is_emitter(g)) return v3(1, 1, 1);
    if (g.Tr > 0) return fresnel_kd ? v3(g.Kd[0], g.Kd[1], g.Kd[2]) : v3(1, 1, 1);
    if (g.Ns > 1) return v3(g.Ks[0], g.Ks[1], g.Ks[2]);
    return v3(g.Kd[0], g.Kd[1], g.Kd[2]);
}

// linear running mean of one channel (running_mean's CVMCTracer branch), both modes
__device__ __forceinline__ float blend_linear(float old, float mean, float pc, float pc1) {
    return (old * pc + mean) / pc1;
}
__device__ __forceinline__ float4 blend_linear4(float4 old, float4 mean, uint32_t prev_count) {
    if (prev_count == 0) return mean;
    const float pc = (float)prev_count, pc1 = (float)(prev_count + 1u);
    return make_float4(blend_linear(old.x, mean.x, pc, pc1), blend_linear(old.y, mean.y, pc, pc1),
                       blend_linear(old.z, mean.z, pc, pc1), blend_linear(old.w, mean.w, pc, pc1));
}

// a-trous B3-spline kernel (Dammertz et al. 2010): 1/16 1/4 3/8 1/4 1/16
__device__ __forceinline__ float atrous_h(int i) {
    return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f);
}

}  // namespace aov
}  // namespace mcpt
