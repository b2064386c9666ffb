// ao_launch.hpp -- ambient-occlusion queries (ao.hip): hemisphere visibility of
// caller-given points (mcpt_ao_device) and of a frame's first hits
// (mcpt_render_ao_device), as an integer count of unoccluded samples per point.
// The lanes make their own rays -- the renders' RNG, sample_lobe and origin
// rule -- and walk them with the any-hit walk of the ray queries (rayquery.hip),
// in a persistent kernel built like it: there is no buffer of rays or flags.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rayquery_launch.hpp"
#include "render_launch.hpp"

namespace mcpt {

// A work unit is (point, run of samples): unit w covers samples
// [r * unit, min((r + 1) * unit, spp)) of point w / upp, r = w % upp.  Point
// form: point i is p[3i..], nrm[3i..], its RNG stream id stream[i] (NULL: i).
// Pixel form (pixel = 1): "point" v is the packed pixel of kp's frame
// (unit_pixel: one shard, whole tiles; padding past the image edge is an empty
// unit), its stream id the pixel's row-major index, and p, nrm, stream unused.
// kp gives scene, spp, spp_offset, key and prev_count to both forms; the frame,
// the camera and best_init to the pixel form.  upp == 1: the lane that ends a
// unit owns its point and writes out[point] itself; else it adds its count to
// counts[point] (zeroed on the stream in front of the kernel) and ao_finish
// forms the floats.  spill as RayQueryParams::spill.
struct AoParams {
    KernelParams kp;
    const float* p;
    const float* nrm;
    const uint32_t* stream;
    float* out;                          // [points] (pixel form: row-major W x H)
    uint32_t* counts;                    // [points] unoccluded samples, upp > 1
    uint4* spill;
    uint32_t spill_stride;
    unsigned long long* stats;           // 8 counters (Counters order)
    uint32_t points;                     // point form: n; pixel form: kp.npix_local
    uint32_t out_n;                      // floats of out: n, or W x H
    uint32_t unit, upp;                  // samples per unit, units per point
    FastDiv div_upp;
    uint32_t total_units;                // points x upp < 2^31
    uint32_t seg;                        // units per workgroup (set by launch_ao)
    int32_t refill;                      // ready lanes before a wave refills (set by launch_ao if 0)
    float radius, bias;                  // resolved: FLT_MAX / 0.01 for the zeros
    int32_t pixel;
};

// Samples per unit and units per point of a query of `points` points x spp: asked > 0
// is taken as given, 0 is one sample per unit (ao.hip has the measurement); either is
// raised only as far as keeps points x upp below 2^31.
struct AoUnits {
    uint32_t unit, upp;
};
AoUnits ao_units(uint64_t points, uint32_t spp, uint32_t asked);
// resolve the scene's kernels on the current device (mcpt_scene_reserve_ao)
hipError_t prepare_ao(const GpuScene& sc);
// counts zeroed (upp > 1), the walk, ao_finish (upp > 1); q.seg and a zero
// q.refill are filled in here.  No points launches nothing.
hipError_t launch_ao(const AoParams& q, bool lean, int cus, int max_workgroups, hipStream_t st);

}  // namespace mcpt
