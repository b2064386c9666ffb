// wf_primary_shade_body.hpp -- the body of wf_primary_shade (wavefront_primary_shade.hip):
// bounce 0 resolved as wf_primary_lists resolves it, and shaded by the wave that
// resolved it.  A group is one 8x8 tile of one sample; its record says how the
// group is resolved (none: every ray misses; up to kListK candidates: pair tests
// from the LDS records; more: the packet walk, wf_primary_walk.hpp), and each
// lane then runs the shade's per-item code (wf_shade_item.hpp) on the ray it
// holds: o = eye, d and the RNG state from the primary_ray call it made, the hit
// id with t, beta, gamma as test_tri_pair left them in its RayState, material and
// list records from the LDS scene image.  Continuing rays go to the head of
// queue 1 and resolved ones to its tail; the kernel's end writes bounce 1's counters as a
// shade does.  In scope: S, BLOCK, kp, wf.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t g = blockIdx.x;
    if (g >= wf.nseg) return;
    const uint32_t count = seg_queue0_len(wf, g);
    if (count == 0) return;                                 // (bounce 1's counters stay the zeros the batch set)
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const GpuScene& sc = kp.scene;
    // LDS: [stack S x BLOCK x 16 B | scene image | counter block: group counter, queue 1's
    // head and tail lengths | the direct lists' record indices], the lean LDS extend's size
    unsigned char* const lds_image = smem + (size_t)S * BLOCK * 16;
    uint32_t* const lgrp = reinterpret_cast<uint32_t*>(lds_image + sc.image_bytes);
    uint32_t& lnext = lgrp[1];
    uint32_t& ltail = lgrp[2];
    uint32_t* const ldk = lgrp + kLdsCounterBytes / 4;
    if (tid < 3) lgrp[tid] = 0;
    if (wf.direct_counts && tid < (int)(kDirectLdsBytes / 4)) ldk[tid] = tid < (int)kDirectTableWords ? wf.direct_list[tid] : 0u;
    MCPT_COPY_SCENE_TO_LDS(lds_image, sc, tid, BLOCK);
    const float4* tris = reinterpret_cast<const float4*>(lds_image + sc.off_tris);
    const uint2* nodes = reinterpret_cast<const uint2*>(lds_image + sc.off_nodes) + 1;
    const uint32_t* leafs = reinterpret_cast<const uint32_t*>(lds_image + sc.off_leafs);
    const GpuGeom* geoms = reinterpret_cast<const GpuGeom*>(lds_image + sc.off_geoms);
    __syncthreads();
    uint4* st = reinterpret_cast<uint4*>(smem) + tid;
    uint4* spill = kp.spill + (blockIdx.x * BLOCK + (uint32_t)tid);
    const uint32_t spill_stride = kp.total_lanes;
    const size_t seg0 = (size_t)g * wf.seg;
    float4* qb2 = wf.q[1];
    const uint32_t qs = wf.slot_stride;
    const int32_t U = BLOCK * 16;                      // one stack position (see slot_of)
    const V3 eye = v3(kp.eye[0], kp.eye[1], kp.eye[2]);
    // what the per-item code reads beside the ray (CV mode only: implicit queue 0)
    constexpr bool SORTB = false, COUNT = false, qe = false;
    const int32_t tdepth = kp.max_depth;
    const uint32_t unlisted = unlisted_boxes(wf.direct_counts);
    Counters c = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t ndirect = 0, nprimary = 0;                 // (wave-uniform) direct rays; paths shaded here
    auto take_group = [&]() {
        uint32_t grp = 0;
        if (lane == 0) grp = atomicAdd(lgrp, 1u);
        return lane_bcast(grp, 0) << 6;
    };
    // the record of the group whose first slot is j0, by scalar loads (wf_primary_body.hpp)
    auto rec_of = [&](uint32_t j0) {
        const uint32_t pid = slot_pid(wf, g, j0);
        const uint32_t u = pid - (pid / wf.nb) * wf.nb;
        return (const_u32*)(wf.tile_cand + (size_t)uni((wf.v0 + u) >> 6) * kListRecWords);
    };
    uint32_t base = take_group();
    const_u32* nrec = (const_u32*)wf.tile_cand;
    u32x4 nh4 = {0u, 0u, 0u, 0u};                       // the next group's {count, first three indices}
    if (base < count) {
        nrec = rec_of(base);
        nh4 = *(const_u32x4*)nrec;
    }
    while (base < count) {
        const uint32_t slot = base + (uint32_t)lane;
        const u32x4 h4 = nh4;
        const_u32* const rec = nrec;
        base = take_group();
        if (base < count) {
            nrec = rec_of(base);
            nh4 = *(const_u32x4*)nrec;
        }
        const uint32_t ncand = uni(h4.x);
        // the lane's path: a slot past the segment's end holds none, one whose pixel lies
        // outside the image ends as the shade ends an empty slot, with a zero by pid
        bool live = slot < count, pix = false;
        uint32_t pid = 0, s_local = 0;
        int px = 0, py = 0;
        if (live) {
            pid = slot_pid(wf, g, slot);
            s_local = pid / wf.nb;
            pix = unit_pixel(kp, wf.v0 + (pid - s_local * wf.nb), px, py);
        }
        if (pix) {
            c.paths++;                                  // (generate's counts)
            c.rays++;
        }
        nprimary += (uint32_t)__popcll(__ballot(pix));
        if (ncand == 0u) {                              // no candidate: every ray of the tile misses
            if (live) stq(&wf.radiance[pid], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            continue;
        }
        RayState r;
        r.o = eye;
        r.d = v3(0, 0, 1);
        r.htri = -1;
        r.best = r.hbeta = r.hgamma = 0.0f;
        uint32_t sd = 0;
        bool active = false, done = false;
        if (pix) {
            primary_ray(kp, (uint32_t)py * (uint32_t)kp.width + (uint32_t)px, px, py, wf.s_begin + s_local, sd, r.d);
            // (the root clip from a per-lane copy of the eye: with the common origin visible the
            // six root-box differences are hoisted out of the group loop into six VGPRs)
            r.o = v3(opaque(eye.x), opaque(eye.y), opaque(eye.z));
            active = begin_ray(r, sc, kp.best_init);
            r.o = eye;
        }
        if (ncand <= kListK) {
#include "wf_primary_pairs.hpp"
        } else {
#include "wf_primary_walk.hpp"
        }
        // ---- the group's 64 lanes shaded in place ----
        uint32_t depth = pix ? 0u : kNoRay;
        V3 o = eye, d = r.d, color = v3(1.0f, 1.0f, 1.0f);
        const float ht = r.best, hb = r.hbeta, hg = r.hgamma;
        const int32_t htri = r.htri;
        int32_t rhit = -1;                              // the hit id of a ray the per-item code resolves
        bool cont = false, direct = false;
        // no carry here: a resolved bounce-1 ray goes to queue 1's tail, where bounce 1's shade
        // takes it (nchain at its bound: the per-item code's carry rule then keeps nothing)
        bool carry = false;
        uint32_t nchain = kCarryMax;
#define MCPT_SHADE_FUSED 1
#include "wf_shade_item.hpp"
#undef MCPT_SHADE_FUSED
    }
    flush_counters(c, kp.stats);
    if (lane == 0 && ndirect) atomicAdd(kp.stats + kStatDirect, (unsigned long long)ndirect);
    if (lane == 0 && nprimary) atomicAdd(kp.stats + kStatPrimaryShaded, (unsigned long long)nprimary);
    __syncthreads();
    if (tid == 0) {
        WfCounters* nx = wf.cnt + (size_t)wf.nseg + g;    // bounce 1's
        nx->queued = lnext;
        nx->resolved = ltail;
    }
