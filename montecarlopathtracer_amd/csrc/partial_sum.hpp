// partial_sum.hpp -- "the partial sum of a unit" as the kernels behind a
// render read it (variance.hip, adaptive.hip; reduce_kernel in render.hip keeps
// its own inline copy of the same lines).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcpt_device.hpp"
#include "render_launch.hpp"

namespace mcpt {

// chunk c's partial sum of pixel v (n samples), as reduce_kernel reads it
__device__ __forceinline__ dev::V3 chunk_partial(const KernelParams& kp, uint32_t c, uint32_t v, uint32_t n) {
    using namespace dev;
    const uint32_t u = c * kp.npix_local + v;
    if (u >= kp.tail_units) {   // tail split: the unit's samples, in sample order
        const float4* tb = kp.tail_buf + (size_t)(u - kp.tail_units) * kp.chunk;
        V3 pc = v3(0, 0, 0);
        for (uint32_t j = 0; j < n; j++) pc = vadd(pc, v3(tb[j].x, tb[j].y, tb[j].z));
        return pc;
    }
    const float4 p = kp.partial[u];
    return v3(p.x, p.y, p.z);
}

}  // namespace mcpt
