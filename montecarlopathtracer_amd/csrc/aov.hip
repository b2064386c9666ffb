// aov.hip -- per-pixel first-hit feature buffers (AOVs) for gfx950: albedo,
// shading normal, depth and coverage of the render's own primary rays.
//
// For sample s of a pixel the ray is the one the path kernels trace first
// (primary_ray / primary_ray_qe: same RNG stream, jitter and reprojection) and
// the closest hit is found by the renders' traversal (begin_ray / trav_iter on
// the scene image in global memory, the top of the stack in LDS, as
// query_kernel).  A hit contributes (albedo, 1) and (shading normal, t), a miss
// zeros; the eight channels are plain fp32 sums in sample order divided by
// (float)spp, then blended into the buffers by the linear running mean when
// prev_count > 0.
//
// Launch shape: 256-thread workgroups stride over the packed pixel order of
// unit_pixel (one shard, tile 8), so each wave holds one 8x8 tile and its rays
// are coherent.  The stack spill area is indexed by launched lane, not by
// pixel: 32 entries x 16 B per lane of at most total_lanes_for() lanes -- the
// area a render of the same scene already holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "aov_device.hpp"
#include "aov_launch.hpp"
#include "mcpt_device.hpp"
#include "render_launch.hpp"
#include "trace_device.hpp"

namespace mcpt {

using namespace dev;
using namespace trace;
using namespace aov;

namespace {

template <bool BOXES, int S, bool QE>
__global__ void __launch_bounds__(kAovBlock) aov_kernel(const KernelParams kp, float4* __restrict__ albedo_cov,
                                                        float4* __restrict__ normal_depth) {
    static_assert((kAovBlock & (kAovBlock - 1)) == 0, "stack slot addresses (slot_of) mask by a power-of-two block");
    __shared__ uint4 stk[S * kAovBlock];   // the only LDS object: slot_of needs the stack at LDS address 0
    const GpuScene& sc = kp.scene;
    const int tid = (int)threadIdx.x;
    const uint32_t gl = blockIdx.x * kAovBlock + (uint32_t)tid;
    const uint32_t lanes = gridDim.x * kAovBlock;               // <= kp.total_lanes (launch_aov)
    const SceneView sv = open_scene<false, kAovBlock>(nullptr, sc, tid);
    uint4* spill = kp.spill + gl;
    const V3 eye = v3(kp.eye[0], kp.eye[1], kp.eye[2]);
    Counters c = {0, 0, 0, 0, 0, 0, 0, 0};   // compiled out (COUNT = false): the scene's stats are not touched
#ifdef MCPT_PHASE_TIMING
    LaneUse lu = {0, 0, 0, 0, 0, 0};
#endif
    const float fspp = (float)kp.spp;

    for (uint32_t v = gl; v < kp.npix_local; v += lanes) {
        int px, py;
        if (!unit_pixel(kp, v, px, py)) continue;               // tile padding past the image edge
        const uint32_t pix = (uint32_t)py * (uint32_t)kp.width + (uint32_t)px;
        float4 ac = make_float4(0, 0, 0, 0), nd = make_float4(0, 0, 0, 0);
        for (uint32_t s = 0; s < kp.spp; s++) {
            uint32_t sd;
            RayState r;
            if constexpr (QE) {
                primary_ray_qe(kp, pix, px, py, s, sd, r.o, r.d);
            } else {
                primary_ray(kp, pix, px, py, s, sd, r.d);
                r.o = eye;
            }
            if (begin_ray(r, sc, kp.best_init))
                while (!trav_iter<S, BOXES, false>(r, sv.tris, sv.nodes, sv.leafs, stk + tid, kAovBlock, spill,
                                                   kp.total_lanes, c MCPT_LU_ARG, sv.pairs)) {
                }
            if (r.htri < 0) continue;                           // a miss adds zeros
            const GpuGeom& g = sv.geoms[__float_as_uint(sv.tris[r.htri + 1].w)];
            // (QuinEngine's scatter never tints a Fresnel bounce, rtx.hlsl:345)
            const V3 alb = first_scatter_albedo(g, QE ? 0 : kp.fresnel_kd);
            V3 n = shading_normal_raw(sc.normals, r.htri, r.hbeta, r.hgamma);
            if constexpr (QE) normalize_hlsl(n);
            else normalize_cu(n);
            ac = make_float4(ac.x + alb.x, ac.y + alb.y, ac.z + alb.z, ac.w + 1.0f);
            nd = make_float4(nd.x + n.x, nd.y + n.y, nd.z + n.z, nd.w + r.best);
        }
        ac = make_float4(ac.x / fspp, ac.y / fspp, ac.z / fspp, ac.w / fspp);
        nd = make_float4(nd.x / fspp, nd.y / fspp, nd.z / fspp, nd.w / fspp);
        const size_t idx = (size_t)py * (size_t)kp.width + (size_t)px;
        if (kp.prev_count) {
            ac = blend_linear4(albedo_cov[idx], ac, kp.prev_count);
            nd = blend_linear4(normal_depth[idx], nd, kp.prev_count);
        }
        albedo_cov[idx] = ac;
        normal_depth[idx] = nd;
    }
}

}  // namespace

hipError_t launch_aov(const KernelParams& kp, float4* albedo_cov, float4* normal_depth, hipStream_t st) {
    if (!kp.npix_local) return hipSuccess;
    const uint32_t want = (kp.npix_local + kAovBlock - 1) / kAovBlock;
    const uint32_t cap = std::max<uint32_t>(kp.total_lanes / kAovBlock, 1u);   // the spill area's lanes
    const dim3 grid(std::min(want, cap));
    const bool qe = kp.mode == kModeQE;
    // stack entries in LDS as query_kernel: 8 for global-memory scenes, 4 for LDS-sized ones
    if (!scene_in_lds(kp.scene)) {
        if (qe) hipLaunchKernelGGL((aov_kernel<true, 8, true>), grid, dim3(kAovBlock), 0, st, kp, albedo_cov, normal_depth);
        else hipLaunchKernelGGL((aov_kernel<true, 8, false>), grid, dim3(kAovBlock), 0, st, kp, albedo_cov, normal_depth);
    } else {
        if (qe) hipLaunchKernelGGL((aov_kernel<false, 4, true>), grid, dim3(kAovBlock), 0, st, kp, albedo_cov, normal_depth);
        else hipLaunchKernelGGL((aov_kernel<false, 4, false>), grid, dim3(kAovBlock), 0, st, kp, albedo_cov, normal_depth);
    }
    return hipGetLastError();
}

}  // namespace mcpt
