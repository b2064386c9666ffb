// adaptive_launch.hpp -- host-side launch interface of the adaptive sampler's
// selection, compaction and merge kernels (adaptive.hip).  The pixel-list
// megakernel itself is render.hip's (launch_render_list).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "render_launch.hpp"

namespace mcpt {

constexpr int kAdaptiveBlock = 256;      // selection / compaction workgroup: 4 waves, 256 packed pixels

// Scene-owned buffers of the adaptive sampler; nblocks = ceil(npix_local / 256)
// of the full frame.
struct AdaptiveWs {
    uint32_t* list;                      // [npix_local] packed pixel indices, ascending
    uint32_t* flags;                     // [width * height] `over` of the current pass, row-major
    uint32_t* blocks;                    // [nblocks + 1] active pixels per block, then their exclusive
                                         // scan; [nblocks] = the list's length
    unsigned long long* masks;           // [nblocks * 4] the waves' ballots of `active`
};
inline uint32_t adaptive_blocks(uint32_t npix_local) { return (npix_local + kAdaptiveBlock - 1) / kAdaptiveBlock; }

// every default resolved
struct AdaptiveSelect {
    float threshold, lum_floor;
    int32_t radius;                      // window radius, 0..4
    uint32_t pass;                       // j >= 1: the pass the list is built for
    int32_t all;                         // 1: no selection -- every pixel of count == j is listed
};

// The list of pass sel.pass on st: `over` per pixel from fb / var (skipped when
// sel.all), active = count == pass and (all or an `over` pixel in the window),
// per-block ballot counts, one-workgroup scan, scatter in ascending packed
// order.  kp: the full frame's KernelParams (tiling).  ws.blocks[nblocks] holds
// the length afterwards.
hipError_t launch_adaptive_select(const KernelParams& kp, const AdaptiveSelect& sel, const AdaptiveWs& ws,
                                  const float4* fb, const float4* var, const uint32_t* count, hipStream_t st);
// Merge of a listed pass: kp is the list kernel's KernelParams (npix_local = the
// list's length, pixel_list, prev_count = j); mean and variance of the pass from
// its partial sums, blended into fb and var as reduce_kernel and
// variance_kernel blend them, count = j + 1.
hipError_t launch_adaptive_merge(const KernelParams& kp, float4* fb, float4* var, uint32_t* count, hipStream_t st);
// count[i] = value for i < n (pass 0 and the full-frame passes)
hipError_t launch_adaptive_fill(uint32_t* count, size_t n, uint32_t value, hipStream_t st);

}  // namespace mcpt
