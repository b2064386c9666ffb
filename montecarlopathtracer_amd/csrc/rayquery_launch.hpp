// rayquery_launch.hpp -- device ray queries (rayquery.hip): closest-hit and
// any-hit of caller-given rays in device memory, through the renders'
// traversal (trace_device.hpp) in a persistent kernel built like the wavefront
// extend (wavefront.hip wf_extend).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "render_launch.hpp"

namespace mcpt {

// Rays i < n: origins / directions as 3 floats each (QueryParams' layout),
// t_max[i] the initial closest t (NULL: best_init for every ray).  Workgroup g
// owns the rays [g * seg, min((g + 1) * seg, n)), seg a multiple of 64.
// Closest hit: tri[i] = tri_order[image slot] (the kd triangle id) or -1,
// hit[3i..] = beta, gamma, t or zeros (hit may be NULL).  Any hit: occ[i] = 1
// once a triangle was accepted with t < t_max.  spill = [32][spill_stride]
// stack entries, indexed by launched lane (the renders' spill area).
struct RayQueryParams {
    GpuScene scene;
    const float* o;
    const float* d;
    const float* t_max;
    int32_t* tri;
    float* hit;
    uint8_t* occ;
    const uint32_t* tri_order;           // image triangle slot -> kd id
    uint4* spill;
    uint32_t spill_stride;
    unsigned long long* stats;           // 8 counters (Counters order)
    uint32_t n;
    uint32_t seg;                        // rays per workgroup (set by launch_rayquery)
    int32_t refill;                      // ready lanes before a wave refills (set by launch_rayquery if 0)
    float best_init;
};

// Fewest rays a workgroup of the automatic grid gets, so the grid shrinks with
// n.  Measured (PERFLOG.md row 171): one wave's 64-ray
// chunk per workgroup is the fastest floor for both layouts -- an LDS-scene
// workgroup's image copy (<= 96 KB by 1024 threads) costs less than walking a
// second chunk of rays on the same CU (2^16 rays, scene01: 256 / 512 / 1024 /
// 2048 rays per workgroup 58 / 64 / 72 / 137 us; 2^10 rays: 64 / 256 / 1024
// 43 / 48 / 48 us).
constexpr uint32_t kRqMinRaysLds = 64;
constexpr uint32_t kRqMinRaysGlobal = 64;

// The schedule of a query of n rays: workgroups and rays per workgroup.
// max_workgroups: 0 = automatic (one per CU for a scene in LDS, the wavefront
// extend's segments per CU for one in global memory), > 0 = at most that many.
struct RayQueryGrid {
    uint32_t workgroups, seg;
};
RayQueryGrid rayquery_grid(const GpuScene& sc, uint32_t n, int cus, int max_workgroups);
// resolve the scene's kernels on the current device (mcpt_scene_reserve_rays)
hipError_t prepare_rayquery(const GpuScene& sc);
// any: the any-hit kernel (writes occ), else closest hit (writes tri, hit);
// lean: traversal counters compiled out.  q.seg and a zero q.refill are filled
// in here.  n = 0 launches nothing.
hipError_t launch_rayquery(const RayQueryParams& q, bool any, bool lean, int cus, int max_workgroups,
                           hipStream_t st);

}  // namespace mcpt
