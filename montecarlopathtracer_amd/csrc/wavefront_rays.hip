// wavefront_rays.hip -- what the wavefront form of the radiance queries
// (mcpt_radiance_ex_device, pipeline = wavefront) adds to the pipeline: the generate
// over the caller's ray buffers, the bounce-0 extend that reads its origins from the
// queue, and the fold of the query's own counter block, with their launches (called
// by wavefront.hip's launch_wavefront and by queries.cpp).  Every later kernel of a ray
// frame is the renders' (render_launch.hpp "Ray frames").  A translation unit of its
// own with wavefront.hip's flags: the instruction streams of the kernels there are
// pinned, and the extend shares its body with them as source text (wf_extend_body.hpp).
#include "wf_device.hpp"

namespace mcpt {
namespace {

constexpr int kRayGenBlock = 256;

// ---- generate over ray buffers ------------------------------------------------
// wf_generate_list's loop -- the dealing of paths to segments, the segments' queue
// lengths, the counters -- over the caller's rays: path pid of the batch is ray
// i = wf.v0 + pid % nb, used as given, sample wf.s_begin + pid / nb.  The RNG starts
// from the ray's stream id in the pixel's place and the two uniforms a render spends
// on its primary ray's jitter are drawn and dropped, as path_body does for the
// megakernel query (render.hip, RAYS).  Queue 0 is explicit: all three streams are
// written.  Every pid < n is a ray; the last group's padding lies past the segment's
// queue length.
// (The names of this unit's kernels must stay clear of the patterns the resource pins
// count the pipeline's kernels by: wf_extend, wf_generate_list, wf_generateE.)
__global__ void __launch_bounds__(kRayGenBlock)
wf_ray_generate(const KernelParams kp, const WfParams wf, const RayInputs ri) {
    const uint32_t n = wf.nb * wf.ns;
    const uint32_t gs = wf.group_shift, gm = (1u << gs) - 1u;
    Counters c = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t pid = blockIdx.x * kRayGenBlock + threadIdx.x; pid < n; pid += gridDim.x * kRayGenBlock) {
        const uint32_t s_local = pid / wf.nb;
        const uint32_t v = wf.v0 + (pid - s_local * wf.nb);
        const uint32_t grp = pid >> gs, blk = grp / wf.nseg;
        const uint32_t g = seg_of(grp - blk * wf.nseg, blk, wf.nseg, wf.xcd_deal);
        const uint32_t slot = g * wf.seg + (blk << gs) + (pid & gm);
        if (grp < wf.nseg && (pid & gm) == 0u) wf.cnt[g].queued = seg_queue0_len(wf, g);   // segment g's queue length
        const uint32_t id = ri.stream ? ri.stream[v] : v;
        const size_t v3i = (size_t)3u * v;
        const V3 o = v3(ri.o[v3i], ri.o[v3i + 1], ri.o[v3i + 2]);
        const V3 d = v3(ri.d[v3i], ri.d[v3i + 1], ri.d[v3i + 2]);
        uint32_t sd = path_seed(kp, id, wf.s_begin + s_local);
        (void)rng_next(sd);
        (void)rng_next(sd);
        c.paths++;
        c.rays++;
        stq(&wf.q[0][qf(slot, kQO, wf.slot_stride)], pack(o, pid));
        stq(&wf.q[0][qf(slot, kQD, wf.slot_stride)], pack(d, 0u));
        stq(&wf.q[0][qf(slot, kQPS, wf.slot_stride)], make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(sd)));
    }
    flush_counters(c, kp.stats);
}

// ---- bounce 0's extend of a ray frame --------------------------------------------
// wf_extend with one change: bounce 0's origins are read from the queue (RAYS0; the
// renders' extend takes them from kp.eye in CV mode).  Same template arguments, launch
// bounds and dynamic LDS as the wf_extend it stands in for; bounces >= 1 are the
// renders' extends.  A bounce-0 ray carries no selector.
template <int LAY, int S, int BLOCK, bool COUNT>
__global__ void __launch_bounds__(BLOCK, (LAY == kLayGlobal && !COUNT && MCPT_WF_GLOBAL_WAVES)
                                             ? MCPT_WF_GLOBAL_WAVES
                                             : (LAY == kLayLds && !COUNT && MCPT_WF_LDS_WPE
                                                    ? MCPT_WF_LDS_WPE : 1))   // (waves per SIMD)
wf_ray_extend0(const KernelParams kp, const WfParams wf) {
    constexpr bool SPHERE = false;
    constexpr bool RAYS0 = true;
    constexpr SphereClip sphc = {};      // (never read: SPHERE is false)
#include "wf_extend_body.hpp"
}

// ---- the query's counter block folded into the scene's ------------------------------
// One wave, plain vector loads and 64-bit atomics as flush_counters': the eight
// Counters of the query's block go to the device or host entry's block (QueryBlocks),
// the routes its rays took to the record mcpt_scene_query_route_rays reports (null for
// the host entry, which reports its own call only)
__global__ void __launch_bounds__(64) wf_ray_fold_stats(const unsigned long long* blk, unsigned long long* counters,
                                                        unsigned long long* routes) {
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)kStatCounters) {
        const unsigned long long v = blk[t];
        if (v) atomicAdd(counters + t, v);
    }
    if (routes && t < (uint32_t)kQueryRoutes) {
        const int slot = t == 0 ? kStatDirect : t == 1 ? kStatExtend : t == 2 ? kStatClipped : kStatSphereSkips;
        const unsigned long long v = blk[slot];
        if (v) atomicAdd(routes + t, v);
    }
}

template <int LAY, int S, int BLOCK>
hipError_t launch_extend0(const KernelParams& kp, const WfParams& wf, int grid, size_t lds, hipStream_t st) {
    auto kern = kp.lean ? wf_ray_extend0<LAY, S, BLOCK, false> : wf_ray_extend0<LAY, S, BLOCK, true>;
    return launch_dyn_lds(kern, dim3(grid), dim3(BLOCK), lds, st, kp, wf);
}

}  // namespace

// This unit's kernels resolved on the current device (part of the reserve: the runtime
// loads a code object at the first use of one of its kernels)
hipError_t load_wavefront_rays() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(wf_ray_generate));
}

hipError_t launch_wavefront_ray_generate(const KernelParams& kp, const WfParams& wf, const RayInputs& ri, int cus,
                                         hipStream_t st) {
    const uint32_t n = wf.nb * wf.ns, grid = (n + kRayGenBlock - 1) / kRayGenBlock, cap = 16u * (uint32_t)cus;
    hipLaunchKernelGGL(wf_ray_generate, dim3(grid < cap ? grid : cap), dim3(kRayGenBlock), 0, st, kp, wf, ri);
    return hipGetLastError();
}

hipError_t launch_wavefront_ray_extend0(const KernelParams& kp, const WfParams& wf, bool in_lds, int grid, size_t lds,
                                        hipStream_t st) {
    return in_lds ? launch_extend0<kLayLds, 4, kLdsBlock>(kp, wf, grid, lds, st)
                  : launch_extend0<kLayGlobal, MCPT_WF_GLOBAL_S, kGlobalBlock>(kp, wf, grid, lds, st);
}

hipError_t launch_wavefront_ray_fold(const unsigned long long* blk, unsigned long long* counters,
                                     unsigned long long* routes, hipStream_t st) {
    hipLaunchKernelGGL(wf_ray_fold_stats, dim3(1), dim3(64), 0, st, blk, counters, routes);
    return hipGetLastError();
}

}  // namespace mcpt
