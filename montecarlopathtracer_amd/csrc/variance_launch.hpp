// variance_launch.hpp -- host-side launch interface of the per-pixel variance
// of a render (variance.hip) and of the variance-guided a-trous denoiser
// (denoise_var.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aov_launch.hpp"
#include "render_launch.hpp"

namespace mcpt {

// variance.hip: batch-means variance of the pixel mean from the partial sums
// (and the tail-split buffer) the render of kp just wrote on the same stream;
// var is row-major, 4 floats per pixel (r g b 0).  kp is the render's resolved
// KernelParams (partial / tail_buf / tail_units set, one shard, not packed,
// nchunks >= 2).  kp.prev_count > 0: var is read and blended.
hipError_t launch_variance(const KernelParams& kp, float4* var, hipStream_t st);

// denoise_var.hip: every default already resolved
struct DenoiseVarParams {
    DenoiseParams base;
    float sigma_l;                       // luminance tolerance in standard deviations, > 0
};
// demodulate (colour, and the luminance variance into alpha) -> `iterations`
// a-trous passes, ping-pong out / scratch as launch_denoise.  color and
// variance are only read.
hipError_t launch_denoise_var(const DenoiseVarParams& p, const float4* color, const float4* variance,
                              const float4* albedo_cov, const float4* normal_depth, float4* out, float4* scratch,
                              hipStream_t st);

}  // namespace mcpt
