// rayquery.hip -- device ray queries (mcpt_trace_device, mcpt_occluded_device):
// closest hit / any hit of caller-given rays in device memory.
//
// The walk is the renders' (trace_device.hpp: begin_ray, then trav_iter until
// it returns true -- what render.hip's query_kernel runs for mcpt_intersect),
// with the scene's own layout; the kernel around it is the wavefront extend's
// (wavefront.hip wf_extend; its layouts and tuning defaults come from
// wf_device.hpp, the scene prologue from trace_device.hpp): persistent
// workgroups, the scene image copied into LDS when it fits (one 1024-thread workgroup per CU) or read through L1/L2
// with the child-box cull (256-thread workgroups, several per CU), the top of
// every lane's stack in LDS.  Workgroup g owns a contiguous range of the rays;
// its waves reserve 64 consecutive rays per LDS atomic, every lane loads its
// next ray a whole burst ahead and takes it as soon as `refill` lanes of its
// wave are done.  No device-wide atomic but the counter flush at the end.
//
// Any hit: a lane is done after the first trav_iter call that leaves a hit.
// Up to there the walk is the closest-hit walk, so occluded[i] == (tri[i] >= 0)
// for the same ray and t_max by construction.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rayquery_launch.hpp"
#include "wf_device.hpp"

namespace mcpt {

namespace {

// The wavefront extend's measured choices (wf_device.hpp), the starting point
// here: descent steps per traversal call, LDS stack entries per lane and the
// waves per SIMD the lean global-memory kernel is held to.
#ifndef MCPT_RQ_DESCENT_CAP
#define MCPT_RQ_DESCENT_CAP MCPT_WF_DESCENT_CAP
#endif
#ifndef MCPT_RQ_DESCENT_CAP_GLOBAL
#define MCPT_RQ_DESCENT_CAP_GLOBAL MCPT_WF_DESCENT_CAP_GLOBAL
#endif
#ifndef MCPT_RQ_GLOBAL_S
#define MCPT_RQ_GLOBAL_S MCPT_WF_GLOBAL_S
#endif
#ifndef MCPT_RQ_GLOBAL_WAVES
#define MCPT_RQ_GLOBAL_WAVES MCPT_WF_GLOBAL_WAVES
#endif
constexpr int kRqLdsS = 4;
static_assert(kRqLdsS <= 4, "scene_in_lds promises room for 4 stack entries per lane");

// a lane's next ray, loaded a burst ahead
struct NextRay {
    float ox, oy, oz, dx, dy, dz, tm;
};

// COUNT = false (lean queries): the traversal counters are compiled out (rays
// are still counted).  ANY: the any-hit query.
template <int LAY, int S, int BLOCK, bool COUNT, bool ANY>
__global__ void __launch_bounds__(BLOCK, (LAY == kLayGlobal && !COUNT) ? MCPT_RQ_GLOBAL_WAVES : 1)   // (waves per SIMD)
rq_trace(const RayQueryParams q) {
    constexpr bool IN_LDS = LAY != kLayGlobal;            // node words in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t first = blockIdx.x * q.seg;            // this workgroup's rays: [first, first + count)
    if (first >= q.n) return;
    const uint32_t count = q.n - first < q.seg ? q.n - first : q.seg;
    const int tid = (int)threadIdx.x;
    const GpuScene& sc = q.scene;
    // LDS: [stack S x BLOCK x 16 B | scene image (kLayLds) | slot counter]
    unsigned char* const lds_image = smem + (size_t)S * BLOCK * 16;
    uint32_t* const lslot = reinterpret_cast<uint32_t*>(lds_image + (IN_LDS ? sc.image_bytes : 0u));
    if (tid == 0) *lslot = 0;
    const SceneView sv = open_scene<IN_LDS, BLOCK>(lds_image, sc, tid);
    __syncthreads();
    uint4* st = reinterpret_cast<uint4*>(smem) + tid;
    uint4* spill = q.spill + (blockIdx.x * BLOCK + (uint32_t)tid);
    const uint32_t spill_stride = q.spill_stride;
    const float* const qo = q.o + (size_t)first * 3;
    const float* const qd = q.d + (size_t)first * 3;
    const float* const qt = q.t_max ? q.t_max + first : nullptr;
    const float best_all = q.best_init;

    Counters c = {0, 0, 0, 0, 0, 0, 0, 0};
#ifdef MCPT_PHASE_TIMING
    LaneUse lu = {0, 0, 0, 0, 0, 0};     // (diagnostic builds: trav_iter's argument, not reported here)
#endif
    SlotCursor cur_chunk = {0, kChunk};
    RayState r;
    r.htri = -1;
    int mode = kDead;
    uint32_t slot = cur_chunk.take(true, lslot);
    uint32_t nslot = cur_chunk.take(true, lslot);
    NextRay nr = {0, 0, 0, 0, 0, 1, 0};
    auto load = [&](uint32_t sl) {
        nr.ox = qo[3 * sl];
        nr.oy = qo[3 * sl + 1];
        nr.oz = qo[3 * sl + 2];
        nr.dx = qd[3 * sl];
        nr.dy = qd[3 * sl + 1];
        nr.dz = qd[3 * sl + 2];
        nr.tm = qt ? qt[sl] : best_all;
    };
    auto start = [&]() {
        // opaque copies: the loop below must not see its ray registers as
        // memory-loaded, or the descent loop's preheader waits for the
        // next-ray prefetch (wf_extend)
        r.o = v3(opaque(nr.ox), opaque(nr.oy), opaque(nr.oz));
        r.d = v3(opaque(nr.dx), opaque(nr.dy), opaque(nr.dz));
        // (no branch: a lane past the end sets a walk up and drops it)
        mode = begin_ray(r, sc, opaque(nr.tm)) ? kTrav : kReady;
    };
    // the refill threshold as an asm result, not a kernel argument read in the
    // loop (a scalar load counted at the loop's exit test, wf_extend)
    int refill;
    asm volatile("s_mov_b32 %0, %1" : "=s"(refill) : "s"(q.refill));
    if (slot < count) {
        load(slot);
        start();
        c.rays++;
    }
    if (nslot < count) load(nslot);
    for (;;) {
        // ---- traversal burst until enough lanes are done -------------------------
        __builtin_amdgcn_s_setprio(0);
        for (;;) {
            if (mode == kTrav) {
                const bool end = trav_iter<S, !IN_LDS, COUNT, LAY == kLayLds,
                                           IN_LDS ? MCPT_RQ_DESCENT_CAP : MCPT_RQ_DESCENT_CAP_GLOBAL>(
                    r, sv.tris, sv.nodes, sv.leafs, st, BLOCK, spill, spill_stride, c MCPT_LU_ARG, sv.pairs);
                if (end || (ANY && r.htri >= 0)) mode = kReady;
            }
            const uint64_t trv = __ballot(mode == kTrav);
            const uint64_t rdy = __ballot(mode == kReady);
            if (!trv || (int)__popcll(rdy) >= refill) break;
        }
        // ---- hand-off: results out, next ray in ----------------------------------
        __builtin_amdgcn_s_setprio(1);
        // the prefetch (issued a whole burst ago) settled before any store of
        // this hand-off: vmcnt counts stores too (wf_extend)
        nr.ox = opaque(nr.ox); nr.oy = opaque(nr.oy); nr.oz = opaque(nr.oz);
        nr.dx = opaque(nr.dx); nr.dy = opaque(nr.dy); nr.dz = opaque(nr.dz);
        nr.tm = opaque(nr.tm);
        const bool fin = mode == kReady;
        if (fin) {
            const uint32_t fslot = slot;
            const int32_t hid = r.htri;
            if constexpr (ANY) {
                slot = nslot;
                start();
                q.occ[(size_t)first + fslot] = hid >= 0 ? 1 : 0;
            } else {
                const float hb = r.hbeta, hg = r.hgamma, ht = hid < 0 ? 0.0f : r.best;
                int32_t id = -1;
                if (hid >= 0) id = (int32_t)q.tri_order[(uint32_t)hid / 3u];
                slot = nslot;
                start();
                const size_t i = (size_t)first + fslot;
                q.tri[i] = id;
                if (q.hit) {
                    q.hit[3 * i] = hb;
                    q.hit[3 * i + 1] = hg;
                    q.hit[3 * i + 2] = ht;
                }
            }
            if (slot >= count) mode = kDead;
            else c.rays++;
        }
        // ---- prefetch the next ray of every lane that just started one -----------
        {
            const bool want = fin && mode != kDead;
            const uint32_t ns = cur_chunk.take(want, lslot);
            if (want) {
                nslot = ns;
                if (nslot < count) load(nslot);
            }
        }
        bound_counters<COUNT>(c, q.stats);
        if (!__ballot(mode != kDead)) break;
    }
    flush_counters(c, q.stats);
}

template <int LAY, int S, int BLOCK>
hipError_t launch_rq(const RayQueryParams& q, bool any, bool lean, uint32_t grid, size_t lds, hipStream_t st) {
    auto kern = any ? (lean ? rq_trace<LAY, S, BLOCK, false, true> : rq_trace<LAY, S, BLOCK, true, true>)
                    : (lean ? rq_trace<LAY, S, BLOCK, false, false> : rq_trace<LAY, S, BLOCK, true, false>);
    return launch_dyn_lds(kern, dim3(grid), dim3(BLOCK), lds, st, q);
}

template <int LAY, int S, int BLOCK>
hipError_t prepare_rq(size_t lds) {
    void (*const kerns[4])(RayQueryParams) = {rq_trace<LAY, S, BLOCK, false, true>, rq_trace<LAY, S, BLOCK, true, true>,
                                              rq_trace<LAY, S, BLOCK, false, false>, rq_trace<LAY, S, BLOCK, true, false>};
    for (auto k : kerns) {
        hipError_t e = set_dyn_lds(k, lds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

// The scene's four kernels resolved on the current device (the runtime loads a
// code object at the first use of one of its kernels, which allocates): part
// of the reserve, so that a query after it allocates nothing.
hipError_t prepare_rayquery(const GpuScene& sc) {
    if (!scene_in_lds(sc)) return prepare_rq<kLayGlobal, MCPT_RQ_GLOBAL_S, kGlobalBlock>(lds_bytes_global(MCPT_RQ_GLOBAL_S, true));
    return prepare_rq<kLayLds, kRqLdsS, kLdsBlock>(lds_bytes_counted_in_lds(sc.image_bytes, kRqLdsS));
}

RayQueryGrid rayquery_grid(const GpuScene& sc, uint32_t n, int cus, int max_workgroups) {
    const bool in_lds = scene_in_lds(sc);
    // never more lanes than the scene's spill area holds (total_lanes_for)
    uint32_t wg = in_lds ? (uint32_t)cus : (uint32_t)cus * (uint32_t)kWfGlobalSegsPerCu;
    if (max_workgroups > 0 && (uint32_t)max_workgroups < wg) wg = (uint32_t)max_workgroups;
    if (wg < 1) wg = 1;
    const uint32_t min_seg = in_lds ? kRqMinRaysLds : kRqMinRaysGlobal;
    uint32_t seg = (uint32_t)((((uint64_t)n + wg - 1) / wg + 63u) & ~(uint64_t)63u);   // whole 64-ray chunks
    if (max_workgroups <= 0 && seg < min_seg) seg = min_seg;   // (an explicit count is taken as given)
    RayQueryGrid g;
    g.seg = seg;
    g.workgroups = (uint32_t)(((uint64_t)n + seg - 1) / seg);
    return g;
}

hipError_t launch_rayquery(const RayQueryParams& q_in, bool any, bool lean, int cus, int max_workgroups,
                           hipStream_t st) {
    if (!q_in.n) return hipSuccess;
    RayQueryParams q = q_in;
    const RayQueryGrid g = rayquery_grid(q.scene, q.n, cus, max_workgroups);
    q.seg = g.seg;
    // the extend's defaults (plan.cpp make_plan wf_refill)
    if (q.refill <= 0) q.refill = scene_in_lds(q.scene) ? 16 : 8;
    if (!scene_in_lds(q.scene))
        return launch_rq<kLayGlobal, MCPT_RQ_GLOBAL_S, kGlobalBlock>(q, any, lean, g.workgroups,
                                                                    lds_bytes_global(MCPT_RQ_GLOBAL_S, true), st);
    return launch_rq<kLayLds, kRqLdsS, kLdsBlock>(q, any, lean, g.workgroups,
                                                  lds_bytes_counted_in_lds(q.scene.image_bytes, kRqLdsS), st);
}

}  // namespace mcpt
