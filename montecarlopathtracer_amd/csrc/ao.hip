// ao.hip -- ambient-occlusion queries (mcpt_ao_device, mcpt_render_ao_device):
// for every point, how many of spp cosine-hemisphere rays of length `radius`
// reach nothing.
//
// The kernel is the ray queries' (rayquery.hip rq_trace, itself the wavefront
// extend's loop): persistent workgroups, the scene image in LDS when it fits
// (one 1024-thread workgroup per CU) or read through L1/L2 with the child-box
// cull (256-thread workgroups), the top of every lane's stack in LDS, 64 work
// units reserved per LDS atomic, a wave refills once `refill` of its lanes are
// done.  What a lane takes is not a ray but a unit (ao_launch.hpp): a point
// and a run of its samples.  It makes each ray itself -- rng_init, the two
// dropped jitter draws, sample_lobe, the scatter's origin rule: the functions
// the renders call -- walks it with the any-hit rule of rq_trace and keeps the
// unit's count of unoccluded samples in a register.  Point form: the lane's
// only loads are the point, the normal and the stream id, prefetched a unit
// ahead.  Pixel form: a sample is two walks of the same lane, the closest hit
// of the render's primary ray (phase 0) and the any-hit walk from it (phase 1);
// a primary miss counts as unoccluded.
//
// Counts are integers: a unit ends with one plain store (the lane owns the
// whole point) or one integer atomic add, so every split of a point's samples
// over lanes, waves and workgroups gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ao_launch.hpp"
#include "aov_device.hpp"
#include "wf_device.hpp"

namespace mcpt {

namespace {

// the ray queries' measured choices (rayquery.hip, from wf_device.hpp)
constexpr int kAoLdsS = 4;
static_assert(kAoLdsS <= 4, "scene_in_lds promises room for 4 stack entries per lane");
// The lean global-memory kernel carries a unit beside its ray: it is held to the
// four waves per SIMD its grid launches (kWfGlobalSegsPerCu workgroups per CU), not
// to the extend's six -- 128 registers, no scratch.
constexpr int kAoGlobalWaves = kWfGlobalSegsPerCu;

// what a lane does at its next hand-off (pixel form: which walk it is on)
constexpr int kPrimary = 0;   // closest hit of the primary ray under way
constexpr int kOccl = 1;      // any-hit walk of an occlusion ray under way
constexpr int kFresh = 2;     // no unit: take one

// the value of a point from its count (the renders' linear running mean, aov_device.hpp)
__device__ __forceinline__ float ao_value(uint32_t unocc, uint32_t spp, uint32_t prev_count, const float* out) {
    const float v = (float)unocc / (float)spp;
    if (prev_count == 0) return v;
    return aov::blend_linear(*out, v, (float)prev_count, (float)(prev_count + 1u));
}

// a lane's next point, loaded a unit ahead (point form)
struct NextPoint {
    float px, py, pz, nx, ny, nz;
    uint32_t id;
};

// COUNT = false (lean): the traversal counters are compiled out (rays, paths
// and shades are still counted).  PIX: the pixel form.
template <int LAY, int S, int BLOCK, bool COUNT, bool PIX>
__global__ void __launch_bounds__(BLOCK, (LAY == kLayGlobal && !COUNT) ? kAoGlobalWaves : 1)   // (waves per SIMD)
ao_walk(const AoParams q) {
    constexpr bool IN_LDS = LAY != kLayGlobal;            // node words in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t first = blockIdx.x * q.seg;            // this workgroup's units: [first, first + count)
    if (first >= q.total_units) return;
    const uint32_t count = q.total_units - first < q.seg ? q.total_units - first : q.seg;
    const int tid = (int)threadIdx.x;
    const KernelParams& kp = q.kp;
    const GpuScene& sc = kp.scene;
    // LDS: [stack S x BLOCK x 16 B | scene image (kLayLds) | slot counter]
    unsigned char* const lds_image = smem + (size_t)S * BLOCK * 16;
    uint32_t* const lslot = reinterpret_cast<uint32_t*>(lds_image + (IN_LDS ? sc.image_bytes : 0u));
    if (tid == 0) *lslot = 0;
    const SceneView sv = open_scene<IN_LDS, BLOCK>(lds_image, sc, tid);
    __syncthreads();
    uint4* st = reinterpret_cast<uint4*>(smem) + tid;
    uint4* spill = q.spill + (blockIdx.x * BLOCK + (uint32_t)tid);
    const uint32_t spill_stride = q.spill_stride;
    const float radius = q.radius;

    Counters c = {0, 0, 0, 0, 0, 0, 0, 0};
#ifdef MCPT_PHASE_TIMING
    LaneUse lu = {0, 0, 0, 0, 0, 0};     // (diagnostic builds: trav_iter's argument, not reported here)
#endif
    SlotCursor cur_chunk = {0, kChunk};
    RayState r;
    r.htri = -1;
    // every lane starts done and without a unit: the first hand-off hands the units out
    int mode = kReady, phase = kFresh;
    uint32_t nslot = cur_chunk.take(true, lslot);
    uint32_t pt = 0;                      // the unit's point (pixel form: the pixel's row-major index)
    uint32_t s = 0, s_end = 0;            // the sample under way, the unit's end
    uint32_t unocc = 0;                   // unoccluded samples of the unit so far
    // point form: the unit's point and the next one's; pixel form: the pixel and the sample's RNG state
    V3 P = v3(0, 0, 0), N = v3(0, 1, 0);
    uint32_t id = 0;
    NextPoint np = {0, 0, 0, 0, 1, 0, 0};
    int px = 0, py = 0;
    uint32_t sd = 1;
    auto load = [&](uint32_t sl) {
        const uint32_t i = q.div_upp.div(first + sl);
        np.px = q.p[3 * (size_t)i];
        np.py = q.p[3 * (size_t)i + 1];
        np.pz = q.p[3 * (size_t)i + 2];
        np.nx = q.nrm[3 * (size_t)i];
        np.ny = q.nrm[3 * (size_t)i + 1];
        np.nz = q.nrm[3 * (size_t)i + 2];
        np.id = q.stream ? q.stream[i] : i;
    };
    if constexpr (!PIX)
        if (nslot < count) load(nslot);
    // the refill threshold as an asm result, not a kernel argument read in the
    // loop (a scalar load counted at the loop's exit test, wf_extend)
    int refill;
    asm volatile("s_mov_b32 %0, %1" : "=s"(refill) : "s"(q.refill));
    for (;;) {
        // ---- traversal burst until enough lanes are done -------------------------
        __builtin_amdgcn_s_setprio(0);
        for (;;) {
            if (mode == kTrav) {
                const bool end = trav_iter<S, !IN_LDS, COUNT, LAY == kLayLds,
                                           IN_LDS ? MCPT_WF_DESCENT_CAP : MCPT_WF_DESCENT_CAP_GLOBAL>(
                    r, sv.tris, sv.nodes, sv.leafs, st, BLOCK, spill, spill_stride, c MCPT_LU_ARG, sv.pairs);
                // any hit: done after the first call that leaves a hit (rq_trace)
                if (end || ((!PIX || phase == kOccl) && r.htri >= 0)) mode = kReady;
            }
            const uint64_t trv = __ballot(mode == kTrav);
            const uint64_t rdy = __ballot(mode == kReady);
            if (!trv || (int)__popcll(rdy) >= refill) break;
        }
        // ---- hand-off: the walk's answer counted, the lane's next ray made ----------
        __builtin_amdgcn_s_setprio(1);
        if constexpr (!PIX) {
            // the prefetch (issued a whole unit ago) settled before any store of
            // this hand-off: vmcnt counts stores too (wf_extend)
            np.px = opaque(np.px); np.py = opaque(np.py); np.pz = opaque(np.pz);
            np.nx = opaque(np.nx); np.ny = opaque(np.ny); np.nz = opaque(np.nz);
        }
        const bool fin = mode == kReady;
        bool newunit = false;
        if (fin) {
            if (PIX && phase == kPrimary && r.htri >= 0) {
                // the diffuse branch of scatter_n at the primary hit, whatever the material
                V3 nrm = shading_normal_raw(sc.normals, r.htri, r.hbeta, r.hgamma);
                normalize_cu(nrm);
                const bool flip = dot3(r.d, nrm) > 0;
                const V3 h = sample_lobe(sd, nrm, false, 0.0f);
                const V3 dir = flip ? v3(-h.x, -h.y, -h.z) : h;
                const V3 hp = v3(r.o.x + r.best * r.d.x, r.o.y + r.best * r.d.y, r.o.z + r.best * r.d.z);
                r.o = vadd(hp, vscale(dir, 0.01f));
                r.d = dir;
                phase = kOccl;
                c.shades++;
                c.rays++;
                mode = begin_ray(r, sc, radius) ? kTrav : kReady;
            } else {
                bool unit_done = true;
                if (phase != kFresh) {
                    unocc += r.htri < 0 ? 1u : 0u;
                    s++;
                    unit_done = s == s_end;
                    if (unit_done) {
                        if (q.upp == 1) q.out[pt] = ao_value(unocc, kp.spp, kp.prev_count, q.out + pt);
                        else if (unocc) atomicAdd(q.counts + pt, unocc);
                    }
                }
                phase = kPrimary;
                if (unit_done) {
                    newunit = true;
                    const uint32_t slot = nslot;
                    if (slot >= count) {
                        mode = kDead;
                    } else {
                        const uint32_t w = first + slot;
                        const uint32_t i = q.div_upp.div(w);
                        s = (w - i * q.upp) * q.unit;
                        const uint32_t left = kp.spp - s;
                        s_end = s + (q.unit < left ? q.unit : left);
                        unocc = 0;
                        if constexpr (PIX) {
                            if (unit_pixel(kp, i, px, py)) {
                                pt = (uint32_t)py * (uint32_t)kp.width + (uint32_t)px;
                            } else {          // tile padding past the image edge: an empty unit
                                phase = kFresh;
                                mode = kReady;
                            }
                        } else {
                            pt = i;
                            P = v3(np.px, np.py, np.pz);
                            N = v3(np.nx, np.ny, np.nz);
                            id = __float_as_uint(opaque(__uint_as_float(np.id)));
                        }
                    }
                }
                if (mode != kDead && phase != kFresh) {
                    c.paths++;
                    c.rays++;
                    if constexpr (PIX) {
                        primary_ray(kp, pt, px, py, s, sd, r.d);
                        r.o = v3(kp.eye[0], kp.eye[1], kp.eye[2]);
                        mode = begin_ray(r, sc, kp.best_init) ? kTrav : kReady;
                    } else {
                        uint32_t sq = rng_init(id, kp.key, kp.spp_offset + s);
                        (void)rng_next(sq);   // the two uniforms a render spends on its jitter
                        (void)rng_next(sq);
                        const float x = rng_next(sq);
                        const float y = rng_next(sq);
                        const V3 h = sample_lobe_u(x, y, N, false, 0.0f);
                        r.o = vadd(P, vscale(h, q.bias));
                        r.d = h;
                        c.shades++;
                        mode = begin_ray(r, sc, radius) ? kTrav : kReady;
                    }
                }
            }
        }
        // ---- reserve (and prefetch) the next unit of every lane that just took one ---
        {
            const bool want = newunit && mode != kDead;
            const uint32_t ns = cur_chunk.take(want, lslot);
            if (want) {
                nslot = ns;
                if constexpr (!PIX)
                    if (nslot < count) load(nslot);
            }
        }
        bound_counters<COUNT>(c, q.stats);
        if (!__ballot(mode != kDead)) break;
    }
    flush_counters(c, q.stats);
}

// out[i] from counts[i] (upp > 1: the units of a point ended in several lanes)
__global__ void __launch_bounds__(256) ao_finish(const uint32_t* __restrict__ counts, float* __restrict__ out,
                                                 uint32_t n, uint32_t spp, uint32_t prev_count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = ao_value(counts[i], spp, prev_count, out + i);
}

template <int LAY, int S, int BLOCK>
hipError_t launch_walk(const AoParams& q, bool lean, uint32_t grid, size_t lds, hipStream_t st) {
    auto kern = q.pixel ? (lean ? ao_walk<LAY, S, BLOCK, false, true> : ao_walk<LAY, S, BLOCK, true, true>)
                        : (lean ? ao_walk<LAY, S, BLOCK, false, false> : ao_walk<LAY, S, BLOCK, true, false>);
    return launch_dyn_lds(kern, dim3(grid), dim3(BLOCK), lds, st, q);
}

template <int LAY, int S, int BLOCK>
hipError_t prepare_walk(size_t lds) {
    void (*const kerns[4])(AoParams) = {ao_walk<LAY, S, BLOCK, false, true>, ao_walk<LAY, S, BLOCK, true, true>,
                                        ao_walk<LAY, S, BLOCK, false, false>, ao_walk<LAY, S, BLOCK, true, false>};
    for (auto k : kerns) {
        hipError_t e = set_dyn_lds(k, lds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

AoUnits ao_units(uint64_t points, uint32_t spp, uint32_t asked) {
    // Automatic: one sample per unit.  A wave's 64 consecutive units are then the
    // samples of a few neighbouring points -- rays from the same origins, walks of
    // similar length -- and every point costs spp integer atomics, the memset and
    // ao_finish.  Measured at 16 spp, lean (profiles/ao/bench.jsonl, DESIGN.md section
    // 15), unit 1 / 4 / 16, ms: scene01 2^20 points 1.73 / 1.94 / 2.57, 2^16 points
    // 0.31 / 0.35 / 0.77; the 70k mesh 2.75 / 2.92 / 3.86 and 0.49 / 0.62 / 1.29.
    uint32_t unit = asked ? asked : 1u;
    if (unit > spp) unit = spp;
    // (scheduling only: a unit is never so short that the units pass 2^31)
    while (unit < spp && points * (((uint64_t)spp + unit - 1) / unit) >= (uint64_t(1) << 31))
        unit = unit < spp / 2 ? unit * 2 : spp;
    return AoUnits{unit, (spp + unit - 1) / unit};
}

hipError_t prepare_ao(const GpuScene& sc) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(ao_finish));
    if (e != hipSuccess) return e;
    if (!scene_in_lds(sc)) return prepare_walk<kLayGlobal, MCPT_WF_GLOBAL_S, kGlobalBlock>(lds_bytes_global(MCPT_WF_GLOBAL_S, true));
    return prepare_walk<kLayLds, kAoLdsS, kLdsBlock>(lds_bytes_counted_in_lds(sc.image_bytes, kAoLdsS));
}

hipError_t launch_ao(const AoParams& q_in, bool lean, int cus, int max_workgroups, hipStream_t st) {
    if (!q_in.total_units) return hipSuccess;
    AoParams q = q_in;
    // the ray queries' grid over the units: workgroups never pass the spill area's lanes
    const RayQueryGrid g = rayquery_grid(q.kp.scene, q.total_units, cus, max_workgroups);
    q.seg = g.seg;
    if (q.refill <= 0) q.refill = scene_in_lds(q.kp.scene) ? 16 : 8;   // (launch_rayquery's defaults)
    hipError_t e = hipSuccess;
    if (q.upp > 1) {
        e = hipMemsetAsync(q.counts, 0, (size_t)q.out_n * 4, st);
        if (e != hipSuccess) return e;
    }
    if (!scene_in_lds(q.kp.scene))
        e = launch_walk<kLayGlobal, MCPT_WF_GLOBAL_S, kGlobalBlock>(q, lean, g.workgroups,
                                                                    lds_bytes_global(MCPT_WF_GLOBAL_S, true), st);
    else
        e = launch_walk<kLayLds, kAoLdsS, kLdsBlock>(q, lean, g.workgroups,
                                                     lds_bytes_counted_in_lds(q.kp.scene.image_bytes, kAoLdsS), st);
    if (e != hipSuccess || q.upp == 1) return e;
    hipLaunchKernelGGL(ao_finish, dim3((q.out_n + 255u) / 256u), dim3(256), 0, st, q.counts, q.out, q.out_n,
                       q.kp.spp, q.kp.prev_count);
    return hipGetLastError();
}

}  // namespace mcpt
