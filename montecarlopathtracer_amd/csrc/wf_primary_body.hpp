// wf_primary_body.hpp -- the body of the wavefront's bounce-0 packet extend,
// included by wavefront_primary.hip into wf_extend_primary (LIST false) and into
// wf_primary_lists (LIST true, COUNT false): the two kernels share the packet
// walk as source text, so the first one's code is the same with and without
// the second (an inlined function changed its epilogue).  In scope: S, BLOCK,
// COUNT, LIST, kp, wf.
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
                if (__ballot(active)) {
                    uint32_t k0 = uni(h4.y), k1n = uni(h4.z);
                    for (uint32_t i = 0; i < ncand; i += 2u) {
                        const bool two = ncand - i >= 2u;
                        const uint32_t k1 = two ? k1n : k0;
                        // (a record has room for one index pair past its last: kListRecWords)
                        const bool more = i + 2u < ncand;
                        const uint32_t j = more ? i : 0u;
                        const uint32_t n0 = rec[j + 3u], n1 = rec[j + 4u];
                        const float4 a0 = ld_tri<true>(tris + k0), a1 = ld_tri<true>(tris + k0 + 1);
                        const float4 a2 = ld_tri<true>(tris + k0 + 2), b0 = ld_tri<true>(tris + k1);
                        const float4 b1 = ld_tri<true>(tris + k1 + 1), b2 = ld_tri<true>(tris + k1 + 2);
                        if (active) test_tri_pair(r, a0, a1, a2, k0, b0, b1, b2, k1, two);
                        k0 = uni(n0);
                        k1n = uni(n1);
                    }
                }
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
        uint32_t w0 = sc.root_w[0], w1 = sc.root_w[1];  // the wave's node
        int32_t sp = 0, lo = 0;                         // wave-uniform stack positions
        if (__ballot(active)) {
            for (;;) {
                if ((w0 >> 30) != 3u) {
                    // ---- inner node: each lane's step of isect_kd_ordered ----
                    if constexpr (COUNT) c.inner += active ? 1u : 0u;
                    const uint32_t left = w0 & kLeftMask;
                    const uint4 pr = *reinterpret_cast<const uint4*>(nodes + left);
                    const int a = (int)(w0 >> 30);
                    const float sv = __uint_as_float(w1);
                    const float oa = sel3(a, eye.x, eye.y, eye.z);   // wave-uniform (common origin)
                    const float ia = sel3(a, r.ix, r.iy, r.iz);
                    const float t = (sv - oa) * ia;
                    const float te = t * kEpsHi;
                    const bool no = !(t > 0.0f) | (t > r.tmax);
                    const bool fo = te < r.tmin;
                    bool first_left, need1, need2;
                    float lo1, hi1, lo2, hi2;
                    if (__builtin_expect(oa != sv, 1)) {
                        // (a uniform branch) the origin is off the plane: every lane's
                        // near side is the wave's first child, below == first_left,
                        // and no lane lies in the plane (pp false)
                        first_left = oa < sv;
                        const bool go_far = !no & fo, both = !no & !fo;
                        need1 = active & !go_far;
                        need2 = active & (go_far | both);
                        // (both interval ends computed unconditionally: a select of the
                        // asm min/max, not a branch around it)
                        const float mn = min_qnan(te, r.tmax), mx = max_qnan(t, r.tmin);
                        lo1 = r.tmin;
                        hi1 = both ? mn : r.tmax;
                        lo2 = go_far ? r.tmin : mx;
                        hi2 = r.tmax;
                    } else {
                        // the origin on the plane: the near side by each lane's direction
                        const float da = sel3(a, r.d.x, r.d.y, r.d.z);
                        const bool below = da <= 0.0f, pp = da == 0.0f;
                        const bool go_far = !pp & !no & fo;
                        const bool push_it = pp | (!pp & !no & !fo);
                        const bool need_near = active & !go_far, need_far = active & (go_far | push_it);
                        const float near_max = push_it ? min_qnan(te, r.tmax) : r.tmax;   // near: [tmin, near_max]
                        const float far_min = go_far ? r.tmin : max_qnan(t, r.tmin);      // far: [far_min, tmax]
                        // the wave's order: left first (the near side of every lane not in the plane)
                        first_left = true;
                        need1 = below ? need_near : need_far;
                        need2 = below ? need_far : need_near;
                        lo1 = below ? r.tmin : far_min;
                        hi1 = below ? near_max : r.tmax;
                        lo2 = below ? far_min : r.tmin;
                        hi2 = below ? r.tmax : near_max;
                    }
                    const uint32_t f0 = first_left ? pr.x : pr.z, f1 = first_left ? pr.y : pr.w;
                    const uint32_t s0 = first_left ? pr.z : pr.x, s1 = first_left ? pr.w : pr.y;
                    if (__ballot(need1)) {
                        if (__ballot(need2)) {                   // push the second child
                            lds_uint4* sl = slot_of<S>(st, BLOCK, sp);
                            if (sp - lo == S * U) {              // LDS part full: its oldest entry to memory
                                spill[((uint32_t)lo / (uint32_t)U) * spill_stride] = ld4(sl);
                                lo += U;
                                if constexpr (COUNT) c.spills++;
                            }
                            st4(sl, make_uint4(s0, s1, __float_as_uint(lo2),
                                               need2 ? __float_as_uint(hi2) : 0x7FC00001u));
                            sp += U;
                        }
                        w0 = f0;
                        w1 = f1;
                        active = need1;
                        r.tmin = lo1;
                        r.tmax = hi1;
                    } else {
                        w0 = s0;
                        w1 = s1;
                        active = need2;
                        r.tmin = lo2;
                        r.tmax = hi2;
                    }
                    continue;
                }
                // ---- leaf: the active lanes test its triangles, two per round ----
                {
                    const uint32_t lpos = w0 & 0x3FFFFFFFu, lend = lpos + w1;
                    if constexpr (COUNT) c.leaf += active ? 1u : 0u;
                    for (uint32_t i = lpos; i < lend; i += 2u) {
                        const bool two = lend - i >= 2u;
                        const uint32_t k0 = leafs[i], k1n = leafs[i + 1u];
                        const uint32_t k1 = two ? k1n : k0;
                        const float4 a0 = ld_tri<true>(tris + k0), a1 = ld_tri<true>(tris + k0 + 1);
                        const float4 a2 = ld_tri<true>(tris + k0 + 2), b0 = ld_tri<true>(tris + k1);
                        const float4 b1 = ld_tri<true>(tris + k1 + 1), b2 = ld_tri<true>(tris + k1 + 2);
                        if (active) {
                            test_tri_pair(r, a0, a1, a2, k0, b0, b1, b2, k1, two);
                            if constexpr (COUNT) {
                                c.refs += two ? 2u : 1u;
                                c.tests += two ? 2u : 1u;
                            }
                        }
                    }
                }
                // ---- pop until an entry with an active lane (or the stack is empty) ----
                bool more = false;
                while (sp > 0) {
                    sp -= U;
                    uint4 e;
                    if (sp < lo) {                               // LDS part empty: the entry is in memory
                        e = settle4(spill[((uint32_t)sp / (uint32_t)U) * spill_stride]);   // (wait here)
                        lo = sp;
                    } else {
                        e = ld4(slot_of<S>(st, BLOCK, sp));
                    }
                    w0 = uni(e.x);
                    w1 = uni(e.y);
                    const float emin = __uint_as_float(e.z), emax = __uint_as_float(e.w);
                    active = false;
                    if ((emax == emax) & !done) {                // this lane's own entry (pop_entry)
                        if (r.best <= emin * kEpsLo) {
                            done = true;                         // its walk ends here
                        } else {
                            active = true;
                            r.tmin = emin;
                            r.tmax = emax;
                        }
                    }
                    if (__ballot(active)) {
                        more = true;
                        break;
                    }
                }
                if (!more) break;
            }
        }
        pslot = slot;
        phit = r.htri;
        base = nbase;
    }
    if (pslot < count) hq[pslot] = phit;
    flush_counters(c, kp.stats);
    if (tid == 0) cn->hits = count;
