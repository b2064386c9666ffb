// wf_extend_body.hpp -- the body of the wavefront's extend kernels as source text,
// included by wavefront.hip into wf_extend (SPHERE false) and by wavefront_sphere.hip
// into wf_sphere_clip (SPHERE true: the lean LDS extend that also cuts a clipped ray's
// walk to its boxes' spheres, render_launch.hpp "Sphere clip").  Source text, not a
// function, so that wf_extend's code stays what it was.  The includer defines LAY, S,
// BLOCK, COUNT and SPHERE (compile-time), has kp and wf as the kernel's arguments and
// sphc, the SphereClip the SPHERE form reads (its kernel argument; wf_extend: none).
// wavefront_rays.hip includes it into wf_ray_extend0 with RAYS0 defined true: bounce 0
// of a ray frame (the wavefront radiance queries), whose origins are the caller's and
// are read from the queue; the other two define it false.
    constexpr bool IN_LDS = LAY != kLayGlobal;            // node words in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t g = blockIdx.x;
    WfCounters* cn = wf.cnt + (size_t)wf.bounce * wf.nseg + g;
    const uint32_t count = g < wf.nseg ? cn->queued : 0u;
    if (count == 0) {
        if (g < wf.nseg && threadIdx.x == 0) cn->hits = 0;
        return;
    }
    const int tid = (int)threadIdx.x;
    const GpuScene& sc = kp.scene;
    // LDS: [stack S x BLOCK x 16 B | scene image (kLayLds) | slot counter]
    unsigned char* const lds_image = smem + (size_t)S * BLOCK * 16;
    uint32_t* const lslot = reinterpret_cast<uint32_t*>(lds_image + (IN_LDS ? sc.image_bytes : 0u));
    if (tid == 0) *lslot = 0;
    const SceneView sv = open_scene<IN_LDS, BLOCK>(lds_image, sc, tid);
    // clip walk (lean renders, scene in LDS): the boxes' triangle lists behind the
    // counter block, for the listed box of a clipped ray's selector, read by the
    // leaf branch as leaf refs -- dtab is the table's word offset from sv.leafs;
    // its last 16 B are zeros (the branch reads the ref after a list's last one:
    // record 0, in bounds, unused)
    constexpr bool CLIP = LAY == kLayLds && !COUNT;
    uint32_t dtab = 0, dcnt = 0;
    if constexpr (CLIP) {
        // (asm results, as the refill threshold below: not kernel-argument reads in the loop)
        asm volatile("s_mov_b32 %0, %1" : "=s"(dcnt) : "s"(wf.direct_counts));
        asm volatile("s_mov_b32 %0, %1" : "=s"(dtab) : "s"((sc.image_bytes + (uint32_t)kLdsCounterBytes - sc.off_leafs) / 4u));
        if (dcnt && tid < (int)(kDirectLdsBytes / 4))
            (lslot + kLdsCounterBytes / 4)[tid] = tid < (int)kDirectTableWords ? wf.direct_list[tid] : 0u;
    }
    // the boxes without a list (a selector's other bit, if any, is its listed
    // box), and this wave's rays started with a selector
    uint32_t unl = 0, nclip = 0, csel = 0;
    if constexpr (CLIP) asm volatile("s_mov_b32 %0, %1" : "=s"(unl) : "s"(unlisted_boxes(wf.direct_counts)));
    // sphere clip: the boxes with a sphere, this wave's selected rays a sphere left no
    // walk, and whether this lane's new ray is one
    uint32_t sph = 0, nskip = 0;
    bool cskip = false;
    if constexpr (SPHERE) asm volatile("s_mov_b32 %0, %1" : "=s"(sph) : "s"(sphc.mask));
    __syncthreads();
    uint4* st = reinterpret_cast<uint4*>(smem) + tid;
    uint4* spill = kp.spill + (blockIdx.x * BLOCK + (uint32_t)tid);
    const uint32_t spill_stride = kp.total_lanes;
    const size_t seg0 = (size_t)g * wf.seg;
    float4* qb = wf.q[wf.bounce & 1];                      // this bounce's queue
    const uint32_t qs = wf.slot_stride;

    Counters c = {0, 0, 0, 0, 0, 0, 0, 0};
#ifdef MCPT_PHASE_TIMING
    LaneUse lu = {0, 0, 0, 0, 0, 0};
#endif
    SlotCursor cur_chunk = {0, kChunk};
    RayState r;
    r.htri = -1;
    int mode = kDead;
    // PF: the next ray of every lane is loaded a whole burst ahead (no4/nd4);
    // without it (MCPT_WF_GLOBAL_PREFETCH = 0, global-memory scenes only) a
    // finished lane loads its next ray in the hand-off, 8 VGPRs fewer
    constexpr bool PF = LAY != kLayGlobal || MCPT_WF_GLOBAL_PREFETCH;
    uint32_t slot = cur_chunk.take(true, lslot), depth = 0;
    uint32_t nslot = PF ? cur_chunk.take(true, lslot) : 0u;
    float4 no4 = make_float4(0, 0, 0, 0), nd4 = make_float4(0, 0, 0, 0);
    auto start = [&](float4 o4, float4 d4) {
        // opaque copies: the loop below must not see its ray registers as
        // memory-loaded, or LLVM flushes vmcnt in the descent loop's preheader
        // (the loop holds the spill store) and waits for the next-ray prefetch
        r.o = v3(opaque(o4.x), opaque(o4.y), opaque(o4.z));
        r.d = v3(opaque(d4.x), opaque(d4.y), opaque(d4.z));
        depth = __float_as_uint(d4.w);
        // (no branch: an empty slot's walk is set up and dropped; begin_ray
        // leaves htri = -1, its miss)
        const bool live = begin_ray(r, sc, kp.best_init);
        // a clipped ray (selector: the mask of the boxes its segment hits): the root
        // interval cut to the union of its unlisted boxes' slab intervals -- the
        // shade's test again, box by box, boxes no lane carries skipped -- and its
        // listed box's triangles, if it has one, tested first by the leaf branch: the
        // root then waits on the stack as the one entry, and the pop behind the list
        // starts the walk or ends the ray (best <= tmin * kEpsLo); an empty interval
        // starts no walk
        if constexpr (CLIP) {
            csel = depth == kNoRay ? 0u : depth >> kDirectShift;
            const uint32_t um = csel & unl;
            const V3 inv = v3(r.ix, r.iy, r.iz);
            float clo = kFltMax, chi = 0.0f;
            float clo0 = kFltMax, chi0 = 0.0f;                // (SPHERE: the union without the spheres)
#pragma unroll 1
            for (uint32_t i = 0; i < wf.n_miss_boxes; i++) {
                const bool mine = ((um >> i) & 1u) != 0u;
                if (((unl >> i) & 1u) != 0u && __ballot(mine)) {
                    float lo, hi;
                    box_interval(r.o, r.d, inv, kp.best_init, wf.miss_box[i], lo, hi);
                    // sphere clip: the box's interval cut to its sphere's; a box with nothing
                    // left -- by the walk's own margins -- adds nothing to the union
                    if constexpr (SPHERE) {
                        clo0 = mine ? min_qnan(clo0, lo) : clo0;
                        chi0 = mine ? max_qnan(chi0, hi) : chi0;
                        if (((sph >> i) & 1u) != 0u) {
                            sphere_interval(r.o, r.d, sphc.sphere[i], lo, hi);
                            const bool none = lo * kEpsLo > hi * kEpsHi;
                            lo = none ? kFltMax : lo;
                            hi = none ? 0.0f : hi;
                        }
                    }
                    clo = mine ? min_qnan(clo, lo) : clo;
                    chi = mine ? max_qnan(chi, hi) : chi;
                }
            }
            const bool sel = csel != 0u;
            const float t0 = max_qnan(r.tmin, clo * kEpsLo);
            const float t1 = min_qnan(r.tmax, (chi * kEpsHi) * kEpsHi);   // (r.tmax: the far end times kEpsHi)
            const bool walk = !(t0 > t1);
            if constexpr (SPHERE)
                cskip = sel && !walk &&
                        !(max_qnan(r.tmin, clo0 * kEpsLo) > min_qnan(r.tmax, (chi0 * kEpsHi) * kEpsHi));
            const uint32_t lm = csel & ~unl;                               // the listed box's bit, or 0
            const bool hasl = lm != 0u;
            const uint32_t lb = (uint32_t)(__ffs((int)lm) - 1) & 7u;
            const uint32_t lp = dtab + lb * kDirectK;
            r.lpos = hasl ? lp : 0u;
            r.lend = hasl ? lp + ((dcnt >> (4u * lb)) & 15u) : 0u;
            r.tmin = sel ? t0 : r.tmin;
            r.tmax = sel ? t1 : r.tmax;
            if (hasl & walk) {
                st4(slot_of<S>(st, BLOCK, 0), make_uint4(r.nw0, r.nw1, __float_as_uint(t0), __float_as_uint(t1)));
                r.sp = BLOCK * 16;
            }
            mode = (depth != kNoRay && live && (!sel | hasl | walk)) ? kTrav : kReady;
            return;
        }
        mode = (depth != kNoRay && live) ? kTrav : kReady;
    };
#ifdef MCPT_PHASE_TIMING
    // the five phase slots (stat_blocks.hpp): setup, traversal bursts, hand-offs, burst iterations, hand-off count
    unsigned long long tm_setup = 0, tm_trav = 0, tm_hand = 0, tm_iters = 0, tm_hands = 0,
                       tm_t0 = __builtin_amdgcn_s_memtime();
#define WF_STAMP(acc) do { unsigned long long t1_ = __builtin_amdgcn_s_memtime(); acc += t1_ - tm_t0; tm_t0 = t1_; } while (0)
#else
#define WF_STAMP(acc) do {} while (0)
#endif
    // the refill threshold as an asm result: a kernel argument read in the
    // loop was a scalar load still counted at the loop's exit test, whose
    // lgkmcnt(0) then also waited for every LDS access in flight, each iteration
    int refill;
    asm volatile("s_mov_b32 %0, %1" : "=s"(refill) : "s"(wf.refill_thresh));
    // MCPT_WF_IMPLICIT0 >= 2: bounce 0's origins are the eye (CV mode), not read
    // (also over a pixel list, whose generate writes the eye into every slot; never
    // in a ray frame's bounce 0, RAYS0)
    const bool eye0 = !RAYS0 && MCPT_WF_IMPLICIT0 >= 2 && wf.bounce == 0 && eye_origins0(kp);
    const float4 eye4 = make_float4(kp.eye[0], kp.eye[1], kp.eye[2], 0.0f);
    auto ld_o = [&](uint32_t sl) { return eye0 ? eye4 : ldq(&qb[qf(seg0 + sl, kQO, qs)]); };
    if (slot < count) start(ld_o(slot), ldq(&qb[qf(seg0 + slot, kQD, qs)]));
    if constexpr (CLIP) nclip += (uint32_t)__popcll(__ballot(slot < count && csel != 0u));
    if constexpr (SPHERE) nskip += (uint32_t)__popcll(__ballot(slot < count && cskip));
    if (PF && nslot < count) { no4 = ld_o(nslot); nd4 = ldq(&qb[qf(seg0 + nslot, kQD, qs)]); }
    WF_STAMP(tm_setup);
    for (;;) {
        // ---- traversal burst until enough lanes are done ---------------------
        __builtin_amdgcn_s_setprio(MCPT_WF_EXT_PRIO);
        for (;;) {
#ifdef MCPT_PHASE_TIMING
            tm_iters++;
            {
                const uint64_t tv = __ballot(mode == kTrav);
                if ((threadIdx.x & 63u) == 0) { lu.burst_w += 1; lu.burst_l += (unsigned long long)__popcll(tv); }
            }
#endif
            MCPT_MARK(5);
            if (mode == kTrav) {
                if (trav_iter<S, !IN_LDS, COUNT, LAY == kLayLds, IN_LDS ? kWfLdsCap : MCPT_WF_DESCENT_CAP_GLOBAL>(
                        r, sv.tris, sv.nodes, sv.leafs, st, BLOCK, spill, spill_stride, c MCPT_LU_ARG, sv.pairs))
                    mode = kReady;
            }
            MCPT_MARK(6);
            const uint64_t trv = __ballot(mode == kTrav);
            const uint64_t rdy = __ballot(mode == kReady);
            if (!trv || (int)__popcll(rdy) >= refill) break;
        }
        WF_STAMP(tm_trav);
#ifdef MCPT_PHASE_TIMING
        tm_hands++;
#endif
        // ---- hand-off: hit id, next ray -----------------------------------
        MCPT_MARK(7);
        __builtin_amdgcn_s_setprio(MCPT_WF_EXT_PRIO + 1);   // as the megakernel's shading rounds: short phase, raised priority
        // Settle the prefetch (issued a whole burst ago) before any store of
        // this hand-off: gfx9's vmcnt also counts stores, so any later wait on
        // the prefetch registers would wait for the stores' acknowledgements.
        // The origin's .w (unused here) is settled too: it keeps its register
        // live across the burst -- a dead load destination is reused by the
        // loop, which must then wait for the load first (a vmcnt wait in every
        // burst's first iteration: C2 +0.9%, C4 +2.8% without it).
        if constexpr (PF) {
            no4 = make_float4(opaque(no4.x), opaque(no4.y), opaque(no4.z), opaque(no4.w));
            nd4 = make_float4(opaque(nd4.x), opaque(nd4.y), opaque(nd4.z), opaque(nd4.w));
        }
        const bool fin = mode == kReady;
        const uint32_t ns0 = PF ? 0u : cur_chunk.take(fin, lslot);   // (collective: every lane)
        const uint32_t fslot = slot;
        csel = 0u;
        cskip = false;
        if (fin) {
            const int32_t hid = r.htri;
            // (the next ray set up unconditionally: no branch in the hand-off; a
            // lane past the segment's end runs on its stale prefetch, then dies)
            if constexpr (PF) {
                slot = nslot;
                start(no4, nd4);
            } else {
                slot = ns0;
                float4 o4 = make_float4(0, 0, 0, 0), d4 = make_float4(0, 0, 0, __uint_as_float(kNoRay));
                if (slot < count) { o4 = ld_o(slot); d4 = ldq(&qb[qf(seg0 + slot, kQD, qs)]); }
                start(o4, d4);
            }
            if (slot >= count) mode = kDead;
            // (r holds the next ray by now: the id saved before)
            reinterpret_cast<int32_t*>(qb + qf(0, kQHIT, qs))[seg0 + fslot] = hid;
        }
        // (wave-uniform: a scalar register; a lane past the segment's end started no ray)
        if constexpr (CLIP) nclip += (uint32_t)__popcll(__ballot(fin && mode != kDead && csel != 0u));
        if constexpr (SPHERE) nskip += (uint32_t)__popcll(__ballot(fin && mode != kDead && cskip));
        // ---- prefetch the next ray of every lane that just started one -------
        if constexpr (PF) {
            const bool want = fin && mode != kDead;
            const uint32_t ns = cur_chunk.take(want, lslot);
            if (want) {
                nslot = ns;
                if (nslot < count) { no4 = ld_o(nslot); nd4 = ldq(&qb[qf(seg0 + nslot, kQD, qs)]); }
            }
        }
        WF_STAMP(tm_hand);
        MCPT_MARK(8);
        if (!__ballot(mode != kDead)) break;
    }
#ifdef MCPT_PHASE_TIMING
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(kp.stats + kStatPhaseUnits, tm_setup);
        atomicAdd(kp.stats + kStatPhaseTrav, tm_trav);
        atomicAdd(kp.stats + kStatPhaseShade, tm_hand);
        atomicAdd(kp.stats + kStatPhaseIters, tm_iters);
        atomicAdd(kp.stats + kStatPhaseScatter, tm_hands);
    }
    {
        unsigned long long* gl = reinterpret_cast<unsigned long long*>(&g_lane_use);
        const unsigned long long v[6] = {lu.desc_w, lu.desc_l, lu.tri_w, lu.tri_l, lu.burst_w, lu.burst_l};
        for (int i = 0; i < 6; i++) {
            unsigned long long x = v[i];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
            if ((threadIdx.x & 63u) == 0) atomicAdd(gl + i, x);
        }
    }
#endif
    flush_counters(c, kp.stats);
    // the rays the secondary extends took (queues past 0 hold no empty slot)
    if (tid == 0 && wf.bounce > 0) atomicAdd(kp.stats + kStatExtend, (unsigned long long)count);
    if constexpr (CLIP)
        if ((tid & 63) == 0 && nclip) atomicAdd(kp.stats + kStatClipped, (unsigned long long)nclip);
    if constexpr (SPHERE)
        if ((tid & 63) == 0 && nskip) atomicAdd(kp.stats + kStatSphereSkips, (unsigned long long)nskip);
    if (tid == 0) cn->hits = count;                        // every slot's hit id is written
