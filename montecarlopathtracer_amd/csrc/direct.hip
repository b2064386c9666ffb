// direct.hip -- direct-lighting queries (mcpt_direct_device, mcpt_render_direct_device):
// for every point, the cosine-weighted mean of the emitter radiance over its
// hemisphere (E / pi), estimated by area sampling of the scene's light table.
//
// The kernel is ao.hip's ao_walk (itself the ray queries' rq_trace): persistent
// workgroups, the scene image in LDS when it fits (one 1024-thread workgroup per
// CU) or read through L1/L2 with the child-box cull (256-thread workgroups), the
// top of every lane's stack in LDS, 64 work units reserved per LDS atomic, a wave
// refills once `refill` of its lanes are done.  A lane takes a unit
// (direct_launch.hpp): a point and one chunk of its samples.  For each sample it
// picks a light by a binary search of the cdf, loads that light's record, makes the
// shadow ray towards a uniform point on it and keeps what the sample adds if
// nothing is in the way as one float, g, beside the light's index; the any-hit walk
// of rq_trace decides, and the next hand-off reads the light's Ka and adds
// g * (Ka * illum) to the unit's sum.  A sample whose point faces away from the
// light's point, or the light's plane from it, or that lies within 2 * bias of it,
// walks nothing and adds nothing.  Pixel form: a sample is two walks of the same
// lane, the closest hit of the render's primary ray (phase 0) and the shadow ray
// from it (phase 1); a primary miss adds nothing.
//
// Sums are floats, so their order is part of the result: a unit's samples are
// added in sample order by the one lane that owns the unit, and the chunk sums in
// chunk order by dl_finish (or, with one chunk, the owning lane forms the value
// itself).  No scheduling field, layout or dealing of units changes a bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "aov_device.hpp"
#include "direct_launch.hpp"
#include "wf_device.hpp"

namespace mcpt {

namespace {

// ao.hip's choices (the ray queries' measured ones, from wf_device.hpp)
constexpr int kDlLdsS = 4;
static_assert(kDlLdsS <= 4, "scene_in_lds promises room for 4 stack entries per lane");
// the lean global-memory kernel is held to the four waves per SIMD its grid launches
// (kWfGlobalSegsPerCu workgroups per CU): 128 registers, no scratch
constexpr int kDlGlobalWaves = kWfGlobalSegsPerCu;

// what a lane does at its next hand-off (pixel form: which walk it is on)
constexpr int kPrimary = 0;   // closest hit of the primary ray under way (point form: a sample under way)
constexpr int kShadow = 1;    // any-hit walk of a shadow ray under way, or a sample without one
constexpr int kFresh = 2;     // no unit: take one

// the value of a point from the sum of its samples: the mean, then the renders'
// linear running mean (render.hip running_mean, CVMCTracer branch)
__device__ __forceinline__ float4 dl_value(V3 sum, uint32_t spp, uint32_t prev_count, const float4* out) {
    const float n = (float)spp;
    const V3 mean = v3(sum.x / n, sum.y / n, sum.z / n);
    if (prev_count == 0) return make_float4(mean.x, mean.y, mean.z, 0.0f);
    const float4 pv = *out;
    const float pc = (float)prev_count, pc1 = (float)(prev_count + 1u);
    return make_float4(aov::blend_linear(pv.x, mean.x, pc, pc1), aov::blend_linear(pv.y, mean.y, pc, pc1),
                       aov::blend_linear(pv.z, mean.z, pc, pc1), 0.0f);
}

// a lane's next point, loaded a unit ahead (point form)
struct NextPoint {
    float px, py, pz, nx, ny, nz;
    uint32_t id;
};

// COUNT = false (lean): the traversal counters are compiled out (rays, paths
// and shades are still counted).  PIX: the pixel form.
template <int LAY, int S, int BLOCK, bool COUNT, bool PIX>
__global__ void __launch_bounds__(BLOCK, (LAY == kLayGlobal && !COUNT) ? kDlGlobalWaves : 1)   // (waves per SIMD)
dl_walk(const DirectParams q) {
    constexpr bool IN_LDS = LAY != kLayGlobal;            // node words in LDS
    // point form: a lane loads its next unit's point a unit ahead -- but for the counting
    // 1024-thread kernel, whose 128 registers have no room for the seven words in flight:
    // it loads the point where it takes the unit
    constexpr bool AHEAD = !PIX && !(COUNT && IN_LDS);
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
    uint32_t dst = 0;                     // where the unit's sum goes: out[point], or partial[chunk * out_n + point]
    uint32_t s = 0, s_end = 0;            // the sample under way, the unit's end
    V3 sum = v3(0, 0, 0);                 // the unit's samples so far
    float g = 0.0f;                       // what the sample under way adds per unit of Ka * illum if unoccluded
    uint32_t lj = 0;                      // ... and its light
    // point form: the unit's point and the next one's; pixel form: the pixel and the sample's RNG state
    V3 P = v3(0, 0, 0), N = v3(0, 1, 0);
    uint32_t id = 0;
    NextPoint np = {0, 0, 0, 0, 1, 0, 0};
    int px = 0, py = 0;
    uint32_t sd = 1;
    auto load = [&](uint32_t sl) {
        const uint32_t i = q.div_chunks.div(first + sl);
        np.px = q.p[3 * (size_t)i];
        np.py = q.p[3 * (size_t)i + 1];
        np.pz = q.p[3 * (size_t)i + 2];
        np.nx = q.nrm[3 * (size_t)i];
        np.ny = q.nrm[3 * (size_t)i + 1];
        np.nz = q.nrm[3 * (size_t)i + 2];
        np.id = q.stream ? q.stream[i] : i;
    };
    // One sample at x with unit normal n from the stream's next three draws: the light,
    // the point on it, the geometry term; the shadow ray into r.  false: nothing to walk
    // (g = 0: no light reaches x from there; or the ray misses the scene's box: unoccluded)
    auto sample = [&](V3 x, V3 n, float bias, uint32_t& sq) -> bool {
        const float u0 = rng_next(sq);
        const float u1 = rng_next(sq);
        const float u2 = rng_next(sq);
        // the first light with u0 < cdf (equal entries: the count of entries <= u0), or the last
        uint32_t lo = 0, hi = q.n_lights;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (q.cdf[mid] <= u0) lo = mid + 1;
            else hi = mid;
        }
        lj = lo < q.n_lights - 1u ? lo : q.n_lights - 1u;
        const float4 a = q.lights[(size_t)lj * kLightRecordVecs];
        const float4 b = q.lights[(size_t)lj * kLightRecordVecs + 1];
        const float4 cc = q.lights[(size_t)lj * kLightRecordVecs + 2];
        const float su = sqrt_rn(u1);
        const float beta = su * (1.0f - u2), gamma = su * u2;
        const V3 y = vadd(vadd(vscale(v3(a.x, a.y, a.z), 1.0f - beta - gamma), vscale(v3(b.x, b.y, b.z), beta)),
                          vscale(v3(cc.x, cc.y, cc.z), gamma));
        const V3 w = vsub(y, x);
        const float r2 = dot3(w, w);
        const float rr = sqrt_rn(r2);
        const V3 dir = v3(w.x / rr, w.y / rr, w.z / rr);
        const float cx = dot3(n, dir);
        const float cy = fabsf(dot3(v3(a.w, b.w, cc.w), dir));
        g = 0.0f;
        r.htri = -1;
        if (!(cx > 0.0f && cy > 0.0f && rr > 2.0f * bias)) return false;
        r.o = vadd(x, vscale(dir, bias));
        r.d = dir;
        g = ((cx * cy) * q.area_total) / (kPwPi * r2);
        c.shades++;
        c.rays++;
        return begin_ray(r, sc, rr - 2.0f * bias);
    };
    if constexpr (AHEAD)
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
                if (end || ((!PIX || phase == kShadow) && r.htri >= 0)) mode = kReady;
            }
            const uint64_t trv = __ballot(mode == kTrav);
            const uint64_t rdy = __ballot(mode == kReady);
            if (!trv || (int)__popcll(rdy) >= refill) break;
        }
        // ---- hand-off: the walk's answer added, the lane's next ray made ------------
        __builtin_amdgcn_s_setprio(1);
        if constexpr (AHEAD) {
            // the prefetch (issued a whole unit ago) settled before any store of
            // this hand-off: vmcnt counts stores too (wf_extend)
            np.px = opaque(np.px); np.py = opaque(np.py); np.pz = opaque(np.pz);
            np.nx = opaque(np.nx); np.ny = opaque(np.ny); np.nz = opaque(np.nz);
        }
        const bool fin = mode == kReady;
        bool newunit = false;
        if (fin) {
            if (PIX && phase == kPrimary && r.htri >= 0) {
                // the primary hit: the shading normal turned against the ray, whatever the material
                V3 nrm = shading_normal_raw(sc.normals, r.htri, r.hbeta, r.hgamma);
                normalize_cu(nrm);
                const bool flip = dot3(r.d, nrm) > 0;
                const V3 n = flip ? v3(-nrm.x, -nrm.y, -nrm.z) : nrm;
                const V3 hp = v3(r.o.x + r.best * r.d.x, r.o.y + r.best * r.d.y, r.o.z + r.best * r.d.z);
                phase = kShadow;
                mode = sample(hp, n, 0.01f, sd) ? kTrav : kReady;
            } else {
                bool unit_done = true;
                if (phase != kFresh) {
                    // (g == 0: a primary miss, or a sample that formed no ray or adds exact zeros)
                    if (r.htri < 0 && g != 0.0f) {
                        const float4 ka = q.lights[(size_t)lj * kLightRecordVecs + 3];
                        sum = vadd(sum, v3(g * (ka.x * q.illum), g * (ka.y * q.illum), g * (ka.z * q.illum)));
                    }
                    s++;
                    unit_done = s == s_end;
                    if (unit_done) {
                        if (q.chunks == 1) q.out[dst] = dl_value(sum, kp.spp, kp.prev_count, q.out + dst);
                        else q.partial[dst] = make_float4(sum.x, sum.y, sum.z, 0.0f);
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
                        const uint32_t i = q.div_chunks.div(w);
                        const uint32_t ck = w - i * q.chunks;
                        s = ck * q.chunk;
                        const uint32_t left = kp.spp - s;
                        s_end = s + (q.chunk < left ? q.chunk : left);
                        sum = v3(0, 0, 0);
                        if constexpr (PIX) {
                            if (unit_pixel(kp, i, px, py)) {
                                dst = ck * q.out_n + ((uint32_t)py * (uint32_t)kp.width + (uint32_t)px);
                            } else {          // tile padding past the image edge: an empty unit
                                phase = kFresh;
                                mode = kReady;
                            }
                        } else {
                            dst = ck * q.out_n + i;
                            if constexpr (!AHEAD) load(slot);
                            P = v3(np.px, np.py, np.pz);
                            N = v3(np.nx, np.ny, np.nz);
                            id = __float_as_uint(opaque(__uint_as_float(np.id)));
                        }
                    }
                }
                if (mode != kDead && phase != kFresh) {
                    c.paths++;
                    if constexpr (PIX) {
                        c.rays++;
                        g = 0.0f;
                        primary_ray(kp, (uint32_t)py * (uint32_t)kp.width + (uint32_t)px, px, py, s, sd, r.d);
                        r.o = v3(kp.eye[0], kp.eye[1], kp.eye[2]);
                        mode = begin_ray(r, sc, kp.best_init) ? kTrav : kReady;
                    } else {
                        uint32_t sq = rng_init(id, kp.key, kp.spp_offset + s);
                        (void)rng_next(sq);   // the two uniforms a render spends on its jitter
                        (void)rng_next(sq);
                        mode = sample(P, N, q.bias, sq) ? kTrav : kReady;
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
                if constexpr (AHEAD)
                    if (nslot < count) load(nslot);
            }
        }
        bound_counters<COUNT>(c, q.stats);
        if (!__ballot(mode != kDead)) break;
    }
    flush_counters(c, q.stats);
}

// out[i] from point i's chunk sums, added in chunk order from 0 (chunks == 0: a
// scene without lights, every sample adds nothing)
__global__ void __launch_bounds__(256) dl_finish(const float4* __restrict__ partial, float4* __restrict__ out,
                                                 uint32_t n, uint32_t chunks, uint32_t spp, uint32_t prev_count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    V3 sum = v3(0, 0, 0);
    for (uint32_t ck = 0; ck < chunks; ck++) {
        const float4 p = partial[(size_t)ck * n + i];
        sum = vadd(sum, v3(p.x, p.y, p.z));
    }
    out[i] = dl_value(sum, spp, prev_count, out + i);
}

template <int LAY, int S, int BLOCK>
hipError_t launch_walk(const DirectParams& q, bool lean, uint32_t grid, size_t lds, hipStream_t st) {
    auto kern = q.pixel ? (lean ? dl_walk<LAY, S, BLOCK, false, true> : dl_walk<LAY, S, BLOCK, true, true>)
                        : (lean ? dl_walk<LAY, S, BLOCK, false, false> : dl_walk<LAY, S, BLOCK, true, false>);
    return launch_dyn_lds(kern, dim3(grid), dim3(BLOCK), lds, st, q);
}

template <int LAY, int S, int BLOCK>
hipError_t prepare_walk(size_t lds) {
    void (*const kerns[4])(DirectParams) = {dl_walk<LAY, S, BLOCK, false, true>, dl_walk<LAY, S, BLOCK, true, true>,
                                            dl_walk<LAY, S, BLOCK, false, false>, dl_walk<LAY, S, BLOCK, true, false>};
    for (auto k : kerns) {
        hipError_t e = set_dyn_lds(k, lds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t prepare_direct(const GpuScene& sc) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(dl_finish));
    if (e != hipSuccess) return e;
    if (!scene_in_lds(sc)) return prepare_walk<kLayGlobal, MCPT_WF_GLOBAL_S, kGlobalBlock>(lds_bytes_global(MCPT_WF_GLOBAL_S, true));
    return prepare_walk<kLayLds, kDlLdsS, kLdsBlock>(lds_bytes_counted_in_lds(sc.image_bytes, kDlLdsS));
}

hipError_t launch_direct(const DirectParams& q_in, bool lean, int cus, int max_workgroups, hipStream_t st) {
    if (!q_in.total_units) return hipSuccess;
    DirectParams q = q_in;
    hipError_t e = hipSuccess;
    if (q.n_lights) {
        // the ray queries' grid over the units: workgroups never pass the spill area's lanes
        const RayQueryGrid g = rayquery_grid(q.kp.scene, q.total_units, cus, max_workgroups);
        q.seg = g.seg;
        if (q.refill <= 0) q.refill = scene_in_lds(q.kp.scene) ? 16 : 8;   // (launch_rayquery's defaults)
        if (!scene_in_lds(q.kp.scene))
            e = launch_walk<kLayGlobal, MCPT_WF_GLOBAL_S, kGlobalBlock>(q, lean, g.workgroups,
                                                                        lds_bytes_global(MCPT_WF_GLOBAL_S, true), st);
        else
            e = launch_walk<kLayLds, kDlLdsS, kLdsBlock>(q, lean, g.workgroups,
                                                         lds_bytes_counted_in_lds(q.kp.scene.image_bytes, kDlLdsS), st);
        if (e != hipSuccess || q.chunks == 1) return e;
    }
    hipLaunchKernelGGL(dl_finish, dim3((q.out_n + 255u) / 256u), dim3(256), 0, st, q.partial, q.out, q.out_n,
                       q.n_lights ? q.chunks : 0u, q.kp.spp, q.kp.prev_count);
    return hipGetLastError();
}

}  // namespace mcpt
