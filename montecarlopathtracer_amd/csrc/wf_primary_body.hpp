// wf_primary_body.hpp -- the body of the wavefront's bounce-0 packet extend,
// included by wavefront_primary.hip into wf_extend_primary (LIST false) and into
// wf_primary_lists (LIST true, COUNT false): the two kernels share the packet
// walk as source text, so the first one's code is the same with and without
// the second (an inlined function changed its epilogue).  The walk itself is
// wf_primary_walk.hpp and a listed group's pair tests are wf_primary_pairs.hpp,
// both of which wf_primary_shade's body includes too.  In scope: S,
// BLOCK, COUNT, LIST, kp, wf.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t g = blockIdx.x;
    WfCounters* cn = wf.cnt + (size_t)wf.bounce * wf.nseg + g;
    uint32_t count = 0;
    if (g < wf.nseg) {
        if constexpr (MCPT_WF_GEN0) {
            count = seg_queue0_len(wf, g);
            if (threadIdx.x == 0) cn->queued = count;          // (read by bounce 0's shade)
        } else {
            count = cn->queued;
        }
    }
    if (count == 0) {
        if (g < wf.nseg && threadIdx.x == 0) cn->hits = 0;
        return;
    }
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const GpuScene& sc = kp.scene;
    // LDS: [stack S x BLOCK x 16 B | scene image | group counter]
    unsigned char* const lds_image = smem + (size_t)S * BLOCK * 16;
    uint32_t* lgrp = reinterpret_cast<uint32_t*>(lds_image + sc.image_bytes);
    if (tid == 0) *lgrp = 0;
    // (the pointers below as they are: taken from open_scene's view, one kernel's branch compiles differently)
    MCPT_COPY_SCENE_TO_LDS(lds_image, sc, tid, BLOCK);
    const float4* tris = reinterpret_cast<const float4*>(lds_image + sc.off_tris);
    const uint2* nodes = reinterpret_cast<const uint2*>(lds_image + sc.off_nodes) + 1;
    const uint32_t* leafs = reinterpret_cast<const uint32_t*>(lds_image + sc.off_leafs);
    __syncthreads();
    uint4* st = reinterpret_cast<uint4*>(smem) + tid;
    uint4* spill = kp.spill + (blockIdx.x * BLOCK + (uint32_t)tid);
    const uint32_t spill_stride = kp.total_lanes;
    const size_t seg0 = (size_t)g * wf.seg;
    float4* qb = wf.q[0];
    const uint32_t qs = wf.slot_stride;
    const int32_t U = BLOCK * 16;                      // one stack position (see slot_of)
    const V3 eye = v3(kp.eye[0], kp.eye[1], kp.eye[2]);
    Counters c = {0, 0, 0, 0, 0, 0, 0, 0};
    __builtin_amdgcn_s_setprio(MCPT_WF_EXT_PRIO);
    // a wave's 64-slot groups: the next group is taken, and its directions
    // loaded, before this one's walk, so the load's latency hides behind it
    auto take_group = [&]() {
        uint32_t grp = 0;
        if (lane == 0) grp = atomicAdd(lgrp, 1u);
        return lane_bcast(grp, 0) << 6;
    };
    // The hits of a group are stored one group later, after the wait for the
    // next directions: a store issued at the end of the walk would make that
    // wait (vmcnt counts stores too) wait for its acknowledgement.
    int32_t* const hq = reinterpret_cast<int32_t*>(qb + qf(0, kQHIT, qs)) + seg0;
    // the primary ray of local slot j: direction and depth (kNoRay: a pixel
    // outside the image, an empty slot)
    auto dir_of = [&](uint32_t j) {
        if constexpr (MCPT_WF_GEN0) {
            const uint32_t pid = slot_pid(wf, g, j);
            const uint32_t s_local = pid / wf.nb;
            int px, py;
            float4 d4 = make_float4(0, 0, 0, __uint_as_float(kNoRay));
            if (unit_pixel(kp, wf.v0 + (pid - s_local * wf.nb), px, py)) {
                uint32_t sd;
                V3 d;
                primary_ray(kp, (uint32_t)py * (uint32_t)kp.width + (uint32_t)px, px, py, wf.s_begin + s_local, sd, d);
                d4 = pack(d, 0u);
                c.paths++;                                      // (generate's counts)
                c.rays++;
            }
            return d4;
        } else {
            return ldq(&qb[qf(seg0 + j, kQD, qs)]);
        }
    };
    uint32_t base = take_group();
    float4 nd4 = make_float4(0, 0, 0, 0);
    // the record of the group whose first slot is j0 (wave-uniform; the groups
    // of a LIST launch are whole tiles: launch_wavefront).  Records are read
    // through the constant address space, i.e. by scalar loads into SGPRs: no
    // wait on them (lgkmcnt) waits for the hit store issued before them, as a
    // vector load's would (vmcnt), and the kernel needs 75 VGPRs, not 80 (the
    // frame time is the same either way).
    auto rec_of = [&](uint32_t j0) {
        const uint32_t pid = slot_pid(wf, g, j0);
        const uint32_t u = pid - (pid / wf.nb) * wf.nb;
        return (const_u32*)(wf.tile_cand + (size_t)uni((wf.v0 + u) >> 6) * kListRecWords);
    };
    const_u32* nrec = (const_u32*)wf.tile_cand;
    u32x4 nh4 = {0u, 0u, 0u, 0u};                       // the next group's {count, first three indices}
    if constexpr (LIST) {
        if (base < count) {
            nrec = rec_of(base);
            nh4 = *(const_u32x4*)nrec;
        }
    } else if (base + (uint32_t)lane < count)
        nd4 = dir_of(base + (uint32_t)lane);
    uint32_t pslot = count;                             // the previous group's slot (count: none)
    int32_t phit = -1;
    for (;;) {
        if (base >= count) break;
        const uint32_t slot = base + (uint32_t)lane;
        uint32_t nbase = 0;
        if constexpr (LIST) {
            const u32x4 h4 = nh4;
            const_u32* const rec = nrec;
            if (pslot < count) hq[pslot] = phit;
            nbase = take_group();
            if (nbase < count) {
                nrec = rec_of(nbase);
                nh4 = *(const_u32x4*)nrec;
            }
            const uint32_t ncand = uni(h4.x);
            if (ncand <= kListK) {
                RayState r;
                r.o = eye;
                r.d = v3(0, 0, 1);
                r.htri = -1;
                bool active = false;
                if (slot < count) {
                    const uint32_t pid = slot_pid(wf, g, slot);
                    const uint32_t s_local = pid / wf.nb;
                    int px, py;
                    if (unit_pixel(kp, wf.v0 + (pid - s_local * wf.nb), px, py)) {
                        c.paths++;                              // (generate's counts)
                        c.rays++;
                        if (ncand != 0u) {
                            uint32_t sd;
                            primary_ray(kp, (uint32_t)py * (uint32_t)kp.width + (uint32_t)px, px, py,
                                        wf.s_begin + s_local, sd, r.d);
                            active = begin_ray(r, sc, kp.best_init);
                        }
                    }
                }
#include "wf_primary_pairs.hpp"
                pslot = slot;
                phit = r.htri;
                base = nbase;
                continue;
            }
            // a longer list: the walk below, its directions made here
            if (slot < count) nd4 = dir_of(slot);
            else nd4 = make_float4(0, 0, 0, __uint_as_float(kNoRay));
        }
        const float4 d4 = make_float4(opaque(nd4.x), opaque(nd4.y), opaque(nd4.z), opaque(nd4.w));
        if constexpr (!LIST) {
            if (pslot < count) hq[pslot] = phit;
            nbase = take_group();
            if (nbase + (uint32_t)lane < count) nd4 = dir_of(nbase + (uint32_t)lane);
        }
        RayState r;
        r.o = eye;
        r.d = v3(0, 0, 1);
        r.htri = -1;
        bool active = false, done = false;
        if (slot < count && __float_as_uint(d4.w) != kNoRay) {
            r.d = xyz(d4);
            active = begin_ray(r, sc, kp.best_init);
        }
#include "wf_primary_walk.hpp"
        pslot = slot;
        phit = r.htri;
        base = nbase;
    }
    if (pslot < count) hq[pslot] = phit;
    flush_counters(c, kp.stats);
    if (tid == 0) cn->hits = count;
