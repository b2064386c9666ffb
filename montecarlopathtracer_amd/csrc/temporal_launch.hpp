// temporal_launch.hpp -- host-side launch interface of the temporal
// accumulation (temporal.hip): a frame's history reprojected onto a new camera.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "render_launch.hpp"

namespace mcpt {

// temporal.hip: every default already resolved (mcpt_temporal_params' zeros replaced)
struct TemporalParams {
    int32_t width, height;
    int32_t mode;                        // MCPT_MODE_*, of both frames
    int32_t gamma_space;
    float max_n;                         // (float)(max_history - 1): the cap on the history length blended in
    float normal_threshold, sigma_z;
    float Wf, Hf, hw;                    // (float)width, (float)height, Hf / Wf
    CameraConsts cur, prev;              // the two frames' cameras
};

// One kernel.  Every buffer is row-major, 4 floats per pixel; var, hist_var and
// out_var are given together or all null (no variance carried).  The inputs
// are only read; the outputs overlap nothing.
hipError_t launch_temporal(const TemporalParams& p, const float4* color, const float4* var, const float4* albedo_cov,
                           const float4* normal_depth, const float4* hist_color_n, const float4* hist_var,
                           const float4* hist_albedo_cov, const float4* hist_normal_depth, float4* out_color_n,
                           float4* out_var, hipStream_t st);

}  // namespace mcpt
