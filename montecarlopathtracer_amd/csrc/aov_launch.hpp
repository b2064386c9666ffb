// aov_launch.hpp -- host-side launch interface of the first-hit feature
// buffers (aov.hip) and the edge-avoiding a-trous denoiser (denoise.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "render_launch.hpp"

namespace mcpt {

// aov.hip: 256-thread workgroups, one wave per 8x8 pixel tile
constexpr int kAovBlock = 256;
// First-hit features of kp's frame (one shard, tile 8, kp.spill = 32 x
// kp.total_lanes stack entries): albedo_cov / normal_depth, row-major, 4 floats
// per pixel.  At most kp.total_lanes lanes are launched.
hipError_t launch_aov(const KernelParams& kp, float4* albedo_cov, float4* normal_depth, hipStream_t st);

// denoise.hip: every default already resolved (mcpt_denoise_params' zeros replaced)
struct DenoiseParams {
    int32_t width, height;
    int32_t iterations;                  // 1..8
    int32_t normal_power_log2;           // 0..10: the normal weight is squared this many times
    float sigma_z, albedo_floor;
    int32_t gamma_space;
};
// demodulate -> `iterations` a-trous passes (ping-pong out / scratch, the last
// one lands in out and remodulates).  color is only read.
hipError_t launch_denoise(const DenoiseParams& p, const float4* color, const float4* albedo_cov,
                          const float4* normal_depth, float4* out, float4* scratch, hipStream_t st);

}  // namespace mcpt
