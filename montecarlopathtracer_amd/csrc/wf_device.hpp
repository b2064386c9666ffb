// wf_device.hpp -- what the wavefront pipeline's translation units share:
// wavefront.hip (generate, extend, shade, cull, candidates, accumulate and the
// host pipeline), wavefront_primary.hip (bounce 0's packet extend and its
// primary-list form, compiled with flags of their own) and
// wavefront_primary_shade.hip (the list form that also shades bounce 0).  The queue layout, the
// dealing of paths to segments, the MCPT_WF_* tuning macros with their
// measurements (those the host's route reads: wf_route.hpp), and the two
// launch entry points of wavefront_primary.hip.
// rayquery.hip takes the extend's layouts and tuning defaults from here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mcpt_device.hpp"
#include "render_launch.hpp"
#include "trace_device.hpp"
#include "wf_route.hpp"

namespace mcpt {

using namespace dev;
using namespace trace;

// wavefront_primary.hip: bounce 0's packet extend of an LDS scene, and the same
// resolving its groups from the per-tile candidate lists (launch_wavefront calls them)
hipError_t launch_wavefront_primary(const KernelParams& kp, const WfParams& wf, int grid, size_t lds,
                                    hipStream_t st);
hipError_t launch_wavefront_primary_lists(const KernelParams& kp, const WfParams& wf, int grid, size_t lds,
                                          hipStream_t st);
// ... and the list form that also shades bounce 0 (lds: the lean LDS extend's with its direct table)
hipError_t launch_wavefront_primary_shade(const KernelParams& kp, const WfParams& wf, int grid, size_t lds,
                                          hipStream_t st);
// wavefront_sphere.hip: the lean LDS extend that cuts a clipped ray's walk to its
// boxes' spheres (lds: the lean LDS extend's)
hipError_t launch_wavefront_sphere_clip(const KernelParams& kp, const WfParams& wf, const SphereClip& clip, int grid,
                                        size_t lds, hipStream_t st);
hipError_t load_wavefront_sphere_clip();   // (its code object loaded now)
// wavefront_rays.hip: a ray frame's generate over the caller's ray buffers and its
// bounce-0 extend, which reads its origins from the queue (lds: WfRoute::extend_lds)
hipError_t launch_wavefront_ray_generate(const KernelParams& kp, const WfParams& wf, const RayInputs& ri, int cus,
                                         hipStream_t st);
hipError_t launch_wavefront_ray_extend0(const KernelParams& kp, const WfParams& wf, bool in_lds, int grid, size_t lds,
                                        hipStream_t st);

namespace {

// Rays are carried as (o.xyz, pid) and (d.xyz, depth); depth kNoRay marks a
// queue slot without a ray (pixel outside the image): it ends as a miss with
// zero radiance and is counted nowhere, like the megakernel's empty units.
constexpr uint32_t kNoRay = 0xFFFFFFFFu;
// Clip walk (render_launch.hpp "Clip walk"): the word's top byte carries a walking
// ray's selector, the mask of the boxes it hits (0 = the full walk); the depth is
// the rest
__device__ __forceinline__ uint32_t ray_depth(uint32_t w) { return w == kNoRay ? w : (w & kDepthMask); }

// Clip walk: the occluder boxes without a list as a mask, bit i box i, from
// WfParams::direct_counts (wave-uniform: scalar operations); 0 for a render
// without lists, whose shades then make no selector
__device__ __forceinline__ uint32_t unlisted_boxes(uint32_t direct_counts) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t b = 0; b < (uint32_t)kMaxMissBoxes; b++) m |= ((direct_counts >> (4u * b)) & 15u) ? 0u : 1u << b;
    return direct_counts ? m : 0u;
}

// Terminal cull (render_launch.hpp "Terminal cull"): can the terminal query's
// ray (o, d) add radiance?  QE: never (its hit is not read); CV: only if its
// closest hit can lie on an emitter (emitter_reachable, reciprocals as
// begin_ray computes them).  The one rule of the shade that makes such a ray
// and of wf_cull_terminal.
__device__ __forceinline__ bool terminal_ray_adds(bool qe, V3 o, V3 d, float best_init,
                                                  const uint32_t (&boxes)[kMaxCullBoxes][3], uint32_t n) {
    if (qe) return false;
    return emitter_reachable(o, d, v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), best_init, boxes, n);
}

// Carry (render_launch.hpp "Direct resolve"): how many times in a row a lane of
// the queue-order shade may keep the ray it resolved instead of writing it to
// the next queue's tail (~0u: no bound).  C2 on two streams of 2^28, ms per
// frame, three runs each: 1 142.4-143.1, 2 144.2-145.8, unbounded 144.7-145.2,
// 0 (no carry; its best schedule, 4 x 2^27) 147.1-147.2 (PERFLOG row 184): a
// longer chain moves more of the frame's shading into the first bounces' kernels
constexpr uint32_t kCarryMax = 1;

__device__ __forceinline__ float4 pack(V3 v, uint32_t w) { return make_float4(v.x, v.y, v.z, __uint_as_float(w)); }

// Queue layout: field k of slot j (kQO {o, pid}, kQD {d, depth}, kQPS
// {throughput, rng}: SoA float4 streams of slot_stride entries each, then
// kQHIT, the 4-B hit ids) -- extend's ray reads and hit writes are dense lane
// streams (64-B AoS records: generate 9 -> 33 ms per C2 frame, round 2).
// WfParams::sort (mcpt_render_params::wf_sort): 0 (default) -- shade takes its
// segment's queue in slot order, dense streams, the merged samplers absorbing
// the material mix; 1 -- shade sorts each block of slots by material first
// (wf_shade_slots SORTB).  Either way continuing rays go to the next queue
// with one LDS atomic per wave.  (Until round 6 the sort went through
// per-class slot lists that extend appended to and shade gathered from: 9.5
// against 13.6 G rays/s for the block sort on C2, PERFLOG row 156.)
__device__ __forceinline__ size_t qf(uint32_t slot, uint32_t k, uint32_t stride) {
    return (size_t)k * stride + slot;
}
// queue streams: origin + path id, direction + depth, throughput + RNG state,
// hit (last: it holds only 4-B triangle ids, so the queue is 3 x 16 + 4 B per
// slot)
constexpr uint32_t kQO = 0, kQD = 1, kQPS = 2, kQHIT = 3;
__device__ __forceinline__ V3 xyz(float4 v) { return v3(v.x, v.y, v.z); }

// Queue streams are touched once per bounce: MCPT_WF_NT marks the streaming
// reads (bit 0) and writes (bit 1) of generate, shade and extend's ray reads
// non-temporal, so that they do not push extend's partially written hit lines
// out of the L2.  Default 3 (C2 wavefront +3.5%, C4 +2%; the 4-B hit ids
// themselves are plain stores, PERFLOG row 79).
#ifndef MCPT_WF_NT
#define MCPT_WF_NT 3
#endif
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ldq(const float4* p) {
#if MCPT_WF_NT & 1
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
__device__ __forceinline__ void stq(float4* p, float4 v) {
#if MCPT_WF_NT & 2
    const f32x4 x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(p));
#else
    *p = v;
#endif
}

// Group k of block b (b-th run of nseg consecutive groups) -> its segment:
// every block deals one group to each segment, rotated by a hash of b.  With
// a plain k -> k (an image of 2^14 8x8 tiles, 256 segments) each segment got
// the same 64 tiles for every sample -- a fixed stripe of the image, whose
// cost differs from the others' and left CUs idle at the end of every extend.
// WfParams::xcd_deal (global-memory scenes, MCPT_WF_XCD): the rotation is a
// multiple of 8, so group k of every block goes to a segment g = k (mod 8).
// Extend and shade workgroup g (one per segment) is dispatched to XCD g mod 8,
// and a group's image region (a 1024x16 strip of 2^14 paths) is k mod (regions
// per sample): every sample of a region then runs on the same XCD, whose L2
// and the caches behind it serve the part of the scene image that region's
// paths walk.  C4 +1.6% (9.31 / 9.34 -> 9.48 / 9.48 G rays/s; serialized
// extends 880 -> 771 ms per two frames at the same L2 hit rate, 0.776 /
// 0.778); LDS scenes keep the finer rotation (C2 -2.3% with it: the coarser
// rotation balances the segments' work less well).
#ifndef MCPT_WF_XCD
#define MCPT_WF_XCD 1
#endif
__device__ __forceinline__ uint32_t seg_of(uint32_t k, uint32_t b, uint32_t nseg, bool xcd) {
    const uint32_t rot = (MCPT_WF_XCD && xcd && (nseg & 7u) == 0u)
                             ? (uint32_t)(((uint64_t)(b * 2654435761u) * (nseg >> 3)) >> 32) << 3
                             : (uint32_t)(((uint64_t)(b * 2654435761u) * nseg) >> 32);
    const uint32_t g = k + rot;
    return g >= nseg ? g - nseg : g;
}

// Inverse of generate's dealing: path id of local slot j of segment g's queue 0.
__device__ __forceinline__ uint32_t slot_pid(const WfParams& wf, uint32_t g, uint32_t j) {
    const uint32_t gs = wf.group_shift, blk = j >> gs;
    const uint32_t rot = seg_of(0, blk, wf.nseg, wf.xcd_deal);
    const uint32_t k = g >= rot ? g - rot : g + wf.nseg - rot;
    return ((blk * wf.nseg + k) << gs) | (j & ((1u << gs) - 1u));
}

// Length of segment g's queue 0 for the batch: its whole groups (the last
// group of the batch may be partial).  Written by generate, or by the
// generate-free bounce-0 extend (MCPT_WF_GEN0).
__device__ __forceinline__ uint32_t seg_queue0_len(const WfParams& wf, uint32_t g) {
    const uint32_t n = wf.nb * wf.ns;
    const uint32_t gs = wf.group_shift, gm = (1u << gs) - 1u;
    const uint32_t ngroups = (n + gm) >> gs;
    const uint32_t full = ngroups / wf.nseg, rem = ngroups - full * wf.nseg;
    // block `full` (partial, rem groups) covers segments rot, rot+1, ... (mod nseg)
    const uint32_t k = (g + wf.nseg - seg_of(0, full, wf.nseg, wf.xcd_deal)) % wf.nseg;
    uint32_t len = (full + (k < rem ? 1u : 0u)) << gs;
    const uint32_t lb = (ngroups - 1u) / wf.nseg;            // block of the last group
    if (seg_of(ngroups - 1u - lb * wf.nseg, lb, wf.nseg, wf.xcd_deal) == g) len -= (ngroups << gs) - n;
    return len;
}

// (MCPT_WF_IMPLICIT0, MCPT_WF_PACKET0, MCPT_WF_GEN0 and the defaults of
// MCPT_WF_GLOBAL_S, MCPT_WF_SHADE_LDS_BLOCK and MCPT_WF_GEO_LDS: wf_route.hpp,
// whose host conditions read them)
// CV mode: every primary ray starts at the eye -- what the extend's bounce 0
// asks before it takes its origins from the kernel arguments (level 2)
__host__ __device__ __forceinline__ bool eye_origins0(const KernelParams& kp) {
    return MCPT_WF_IMPLICIT0 && kp.mode != kModeQE;
}
// A frame over a pixel list (adaptive sampling's listed passes, wf_generate_list)
// has an explicit queue 0: the slot gives the list index, not the pixel, so
// generate writes all three streams, the host launches no packet extend and the
// shade reads its state.  (A test of a kernel argument: a scalar compare.)  Its
// origins are the eye all the same: the extend keeps eye_origins0 and its code.
// The pointer also marks "explicit queue 0" for a ray frame (the wavefront radiance
// queries, render_launch.hpp "Ray frames"): its host sets a non-null pixel_list that
// no kernel of its route dereferences, so the shades read bounce 0's state from the
// queue; its origins are the caller's, and its bounce 0 has an extend of its own.
__host__ __device__ __forceinline__ bool implicit0(const KernelParams& kp, const WfParams& wf) {
    return eye_origins0(kp) && kp.pixel_list == nullptr;
}
// Hit ids: extend writes only the hit triangle's id (4 B, the
// first quarter of the hit stream as i32) and shade recomputes t, beta, gamma
// of a scattering ray from it (tri_hit_params: the traversal's own
// operations, bit-identical).  The 16-B hit records cost the extend 2.4x their
// bytes in partly written L2 lines; C2 wavefront +3.7% (12.70 -> 13.18, three
// rounds), C4 +2.8%.  (plan.cpp wf_layout sizes the queues for this.)

// Issue priority of the extend's traversal bursts (its hand-off runs one
// higher); the co-resident shade runs at 0.
#ifndef MCPT_WF_EXT_PRIO
#define MCPT_WF_EXT_PRIO 0
#endif

// Descent steps per traversal call in the wavefront extend (the megakernel's
// MCPT_DESCENT_CAP is 4): with shading out of the loop a longer descent burst
// pays (C2 wf cap 3 / 4 / 5 / 6: 13.57 / 13.64 / 13.84 / 13.57 G rays/s)
#ifndef MCPT_WF_DESCENT_CAP
#define MCPT_WF_DESCENT_CAP 5
#endif
// Global-memory scenes: 6 since round 6's cheaper descent step (C4 cap
// 4 / 5 / 6 / 7: 10.84 / 11.19 / 11.40 / 11.06 and 10.86 / 11.14 / 11.30 /
// 11.05 G rays/s, PERFLOG row 164); the megakernel keeps MCPT_DESCENT_CAP_GLOBAL
#ifndef MCPT_WF_DESCENT_CAP_GLOBAL
#define MCPT_WF_DESCENT_CAP_GLOBAL 6
#endif
constexpr int kWfLdsCap = MCPT_WF_DESCENT_CAP;

// Residency of the global-memory extend (C4: a walk bound by the latency of
// node and triangle reads from L2 / MALL, so every resident wave counts).
// Workgroups of 256 threads, kGlobalBlocksPerCu per CU per launch; other
// streams' extends fill further slots as far as LDS and VGPRs allow.
// MCPT_WF_GLOBAL_S: LDS stack entries per lane; MCPT_WF_GLOBAL_WAVES: waves per
// SIMD the compiler must allow (its VGPR budget; the lean kernel only -- the
// untimed counting kernels keep their registers) -- with 256-thread
// workgroups (one wave per SIMD each) that is the resident workgroups per CU.
// 6 x 6: 80 VGPRs (no scratch) and 6 x 24 KB of LDS, six extend waves per
// SIMD.  C4 G rays/s:
// S = 8, no hint (round 3: 32 KB, four workgroups, 88 VGPRs) 9.46 / 9.47;
// S = 6 9.61 / 9.63; S = 7 (five workgroups) 9.85 / 9.87; S = 5 9.20; S = 4
// 8.78 (spills); S = 6 with six workgroups (80 VGPRs) 10.36 / 10.31.
#ifndef MCPT_WF_GLOBAL_WAVES
#define MCPT_WF_GLOBAL_WAVES 6
#endif
static_assert(kGlobalBlock == 256, "MCPT_WF_GLOBAL_WAVES = workgroups per CU only for one wave per SIMD each");
#ifndef MCPT_WF_GLOBAL_PREFETCH
#define MCPT_WF_GLOBAL_PREFETCH 1
#endif
// register budget (waves per SIMD the compiler plans for; 0 = none) of the
// LDS scenes' lean extend, and the shade's workgroup beside an LDS extend
// workgroup (512: two waves per SIMD)
#ifndef MCPT_WF_LDS_WPE
#define MCPT_WF_LDS_WPE 0
#endif
// scene layouts of the persistent traversal kernels (wf_extend, rq_trace)
constexpr int kLayGlobal = 0, kLayLds = 1;

__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// read-only words another kernel wrote, at wave-uniform addresses: the
// constant address space (scalar loads; wf_primary_body.hpp)
typedef const __attribute__((address_space(4))) uint32_t const_u32;
typedef const __attribute__((address_space(4))) u32x4 const_u32x4;

}  // namespace
}  // namespace mcpt
