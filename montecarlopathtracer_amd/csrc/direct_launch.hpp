// direct_launch.hpp -- direct-lighting queries (direct.hip): how much emitter light
// reaches caller-given points (mcpt_direct_device) and a frame's first hits
// (mcpt_render_direct_device), by area sampling of the scene's light table.  The
// lanes make their own shadow rays -- the renders' RNG, a light picked from the
// table's cdf, a uniform point on it -- and walk them with the any-hit walk of the
// ray queries (rayquery.hip), in a persistent kernel built like ao.hip's: there is
// no buffer of rays or flags.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rayquery_launch.hpp"
#include "render_launch.hpp"

namespace mcpt {

// One light triangle on the device: four float4
//   [0] v0.xyz, ng.x   [1] v1.xyz, ng.y   [2] v2.xyz, ng.z   [3] Ka.rgb, 0
// (v: the kd triangle's fp32 vertices; ng: its unit geometric normal; Ka: its
// geometry's).  The cdf is an array of its own: cdf[k] = (float)(S_k / S_last).
constexpr uint32_t kLightRecordBytes = 64;
constexpr uint32_t kLightRecordVecs = kLightRecordBytes / 16;

// A work unit is (point, chunk): unit w covers samples [c * chunk, min((c + 1) * chunk,
// spp)) of point w / chunks, c = w % chunks -- the chunks are part of the result (their
// sums are added in chunk order), not of the scheduling.  Point form: point i is
// p[3i..], nrm[3i..], its RNG stream id stream[i] (NULL: i).  Pixel form (pixel = 1):
// "point" v is the packed pixel of kp's frame (unit_pixel: one shard, whole tiles;
// padding past the image edge is an empty unit), its stream id the pixel's row-major
// index, and p, nrm, stream unused.  kp gives scene, spp, spp_offset, key and
// prev_count to both forms; the frame, the camera and best_init to the pixel form.
// chunks == 1: the lane that ends a unit writes out[point] itself; else it stores the
// unit's sum to partial[c * out_n + point] and dl_finish adds them in order.  spill as
// RayQueryParams::spill.
struct DirectParams {
    KernelParams kp;
    const float* p;
    const float* nrm;
    const uint32_t* stream;
    float4* out;                         // [points] r, g, b, 0 (pixel form: row-major W x H)
    float4* partial;                     // [chunks][out_n], chunks > 1
    const float4* lights;                // [n_lights] records of kLightRecordVecs
    const float* cdf;                    // [n_lights], non-decreasing, the last 1.0f
    uint4* spill;
    uint32_t spill_stride;
    unsigned long long* stats;           // 8 counters (Counters order)
    uint32_t points;                     // point form: n; pixel form: kp.npix_local
    uint32_t out_n;                      // float4s of out: n, or W x H
    uint32_t chunk, chunks;              // samples per unit, units per point
    FastDiv div_chunks;
    uint32_t total_units;                // points x chunks < 2^31
    uint32_t seg;                        // units per workgroup (set by launch_direct)
    int32_t refill;                      // ready lanes before a wave refills (set by launch_direct if 0)
    uint32_t n_lights;
    float area_total;                    // (float)(the lights' areas summed in double)
    float illum;
    float bias;                          // resolved: 0.01 for the point form's zero and for the pixel form
    int32_t pixel;
};

// resolve the scene's kernels on the current device (mcpt_scene_reserve_direct)
hipError_t prepare_direct(const GpuScene& sc);
// the walk, then dl_finish (chunks > 1); a scene without lights launches dl_finish
// alone, over no partial sums.  q.seg and a zero q.refill are filled in here.  No
// points launches nothing.
hipError_t launch_direct(const DirectParams& q, bool lean, int cus, int max_workgroups, hipStream_t st);

}  // namespace mcpt
