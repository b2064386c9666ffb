// wf_shade_item.hpp -- the wavefront shade's per-item code and its enqueue: the
// one statement of the path rule for a queued ray with a known hit, included
// as source text by wf_shade_slots (wavefront.hip), which takes the ray from a
// queue slot or from its own carry, and by wf_primary_shade
// (wavefront_primary_shade.hip), which has just resolved it in the same lane.
// Source text, not a function, for the reason wf_primary_body.hpp gives: the
// shade kernels' code stays what it was.
// MCPT_SHADE_FUSED (defined by the including kernel, 0 or 1) says where the
// hit's t, beta, gamma and the records come from:
//   0  t, beta, gamma recomputed from the hit id (tri_hit_params); the direct
//      lists' records in the shade's own copy (ldrec, indices ldk); tris and
//      geoms wherever the kernel reads them from -- in queue order (!SORTB) the
//      hit's own records are the values wf_shade_slots loaded in one group behind
//      the hit id: rt0..rt2 = tris[htri .. htri + 2], rn0..rn2 = normals[htri ..
//      htri + 2] (defined where htri >= 0 in a live lane, the only place read)
//   1 t, beta, gamma as the resolving test_tri_pair left them (ht, hb, hg:
//      RayState::best / hbeta / hgamma); tris and geoms are the LDS scene image's,
//      so the lists' records are tris + ldk[entry] and no copy exists
// In scope: SORTB, kp, wf, sc, qe, tdepth, unlisted, tris, geoms, ldk (ldrec),
// c, ndirect, lane, seg0, qb2, qs, lnext, ltail; per lane: live (the lane holds
// a ray), pid, depth, sd, o, d, color, htri, and the results cont, direct, rhit,
// carry, nchain.
        if (live) {
            float4 h = make_float4(0, 0, 0, 0);
            // CV: miss -> 0; emitter -> color*Ka*ILLUM (:111-113); terminal query
            // (:162-175); else scatter.  QE: miss / bounce >= 3*depth -> 0; roulette
            // from bounce `depth` on; emitter -> color*Ka (rtx.hlsl:312-331)
            V3 L = v3(0, 0, 0);
            bool term = true;
            if (htri >= 0 && depth != kNoRay) {
#if MCPT_SHADE_FUSED
                const GpuGeom& gm = geoms[__float_as_uint(tris[htri + 1].w)];
#else
                uint32_t gi0;                                 // the hit's geometry index
                if constexpr (SORTB) gi0 = __float_as_uint(tris[htri + 1].w);
                else gi0 = __float_as_uint(rt1.w);
                const GpuGeom& gm = geoms[gi0];
#endif
                if (qe) {
                    if ((int32_t)depth < 3 * kp.max_depth &&
                        ((int32_t)depth < kp.max_depth || qe_roulette(sd, color))) {
                        if (is_emitter(gm)) L = emitted(color, gm, 1.0f);
                        else term = false;
                    }
                } else if ((int32_t)depth >= kp.max_depth || is_emitter(gm)) {
                    L = emitted(color, gm, kp.illum);
                } else {
                    term = false;
                }
                if (!term) {
                    c.shades++;
#if MCPT_SHADE_FUSED
                    h = make_float4(ht, hb, hg, 0.0f);
                    if (qe) scatter<true>(gm, sc.normals, htri, h.y, h.z, h.x, 0, sd, color, o, d);
                    else scatter<false>(gm, sc.normals, htri, h.y, h.z, h.x, kp.fresnel_kd, sd, color, o, d);
#else
                    if constexpr (SORTB) {
                        tri_hit_params(o, d, tris[htri], tris[htri + 1], tris[htri + 2], h.x, h.y, h.z);
                        if (qe) scatter<true>(gm, sc.normals, htri, h.y, h.z, h.x, 0, sd, color, o, d);
                        else scatter<false>(gm, sc.normals, htri, h.y, h.z, h.x, kp.fresnel_kd, sd, color, o, d);
                    } else {   // (scatter is these loads, then scatter_n)
                        tri_hit_params(o, d, rt0, rt1, rt2, h.x, h.y, h.z);
                        if (qe) scatter_n<true>(gm, rn0, rn1, rn2, h.y, h.z, h.x, 0, sd, color, o, d);
                        else scatter_n<false>(gm, rn0, rn1, rn2, h.y, h.z, h.x, kp.fresnel_kd, sd, color, o, d);
                    }
#endif
                    cont = true;
                    c.rays++;
                    // the new ray against the scene's occluder boxes (lean renders:
                    // n_miss_boxes != 0), in this order: box test, cull, direct, resolve,
                    // clip selector
                    // (o and d settled: only they, the throughput, the RNG state and pid are
                    // live here, but with the test's operations free to move up into scatter
                    // the queue-order shade took 81 VGPRs, one over its budget; 79 with this)
                    o = v3(opaque(o.x), opaque(o.y), opaque(o.z));
                    d = v3(opaque(d.x), opaque(d.y), opaque(d.z));
                    if (wf.n_miss_boxes) {
                        // (acc: the mask of the boxes hit)
                        const uint32_t acc = scene_box_hits(o, d, v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), kp.best_init,
                                                            wf.miss_box, wf.n_miss_boxes);
                        // miss cull: the new ray misses every occluder box, so its walk would
                        // return no hit and the next shade would store this zero; the ray stays
                        // counted and is not enqueued
                        if (!acc) {
                            stq(&wf.radiance[pid], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                            cont = false;
                        }
                        // direct lists: a ray that hits one box, and a small one (direct_counts:
                        // 4 bits per box, 0 = walk), can only hit that box's list
                        const uint32_t box = (uint32_t)(__ffs((int)acc) - 1) & 7u;
                        direct = acc != 0u && (acc & (acc - 1u)) == 0u && ((wf.direct_counts >> (4u * box)) & 15u) != 0u;
                        // direct resolve: the extend's answer for a direct ray, operation for
                        // operation -- begin_ray (its reciprocals are the box test's), then
                        // the box's list in list order, in pairs, records from the LDS copy;
                        // a hit goes to the next queue's tail with its ray, no hit ends the
                        // path with the zero the next shade would store
                        if (direct) {
                            RayState r;
                            r.o = o;
                            r.d = d;
                            if (begin_ray(r, sc, kp.best_init)) {
                                const uint32_t n = (wf.direct_counts >> (4u * box)) & 15u;
#pragma unroll
                                for (uint32_t j = 0; j < kDirectK; j += 2u) {
                                    if (j < n) {
                                        const bool two = n - j >= 2u;
                                        const uint32_t e0 = box * kDirectK + j, e1 = (j + 1u < kDirectK && two) ? e0 + 1u : e0;
                                        const uint32_t k0 = ldk[e0], k1 = ldk[e1];
#if MCPT_SHADE_FUSED
                                        const float4* const ra = tris + k0;
                                        const float4* const rb = tris + k1;
#else
                                        const float4* const ra = ldrec + 3u * e0;
                                        const float4* const rb = ldrec + 3u * e1;
#endif
                                        test_tri_pair<false>(r, ld_tri<true>(ra), ld_tri<true>(ra + 1), ld_tri<true>(ra + 2), k0,
                                                             ld_tri<true>(rb), ld_tri<true>(rb + 1), ld_tri<true>(rb + 2), k1, two);
                                    }
                                }
                            }
                            rhit = r.htri;
                            cont = false;
                            // the terminal query's ray (CV: depth max_depth, QE: 3 * max_depth): the next
                            // shade would only store its hit's emission (QE: zero) -- stored here, so
                            // the last queue has no tail and the ray is neither written nor read again
                            if (rhit >= 0 && (int32_t)(depth + 1u) >= tdepth) {
                                V3 Lt = v3(0, 0, 0);
                                if (!qe) {
                                    uint32_t gi = 0;                  // the hit record's geometry, from the copy
#if MCPT_SHADE_FUSED
                                    gi = __float_as_uint(tris[rhit + 1].w);
#else
#pragma unroll
                                    for (uint32_t j = 0; j < kDirectK; j++)
                                        if (ldk[box * kDirectK + j] == (uint32_t)rhit)
                                            gi = __float_as_uint(ldrec[3u * (box * kDirectK + j) + 1u].w);
#endif
                                    Lt = emitted(color, geoms[gi], kp.illum);
                                }
                                stq(&wf.radiance[pid], make_float4(Lt.x, Lt.y, Lt.z, 0.0f));
                                rhit = -1;
                            } else if (rhit < 0)
                                stq(&wf.radiance[pid], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                        }
                        // terminal cull (wf.shade_cull; render_launch.hpp "Terminal cull"): a walking
                        // ray made for the terminal query that can add no radiance -- wf_cull_terminal's
                        // own rule -- gets the zero its shade would store and is not enqueued; it stays
                        // counted.  (A resolved one was finished above.)
                        if (!SORTB && wf.shade_cull && (qe || wf.n_cull_boxes) && cont && (int32_t)(depth + 1u) == tdepth &&
                            !terminal_ray_adds(qe, o, d, kp.best_init, wf.cull_box, wf.n_cull_boxes)) {
                            stq(&wf.radiance[pid], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                            cont = false;
                        }
                        // clip walk: a walking ray through at least one box without a list and
                        // at most one with a list carries its box mask (never a direct ray, whose
                        // one box has a list, nor a culled one, whose mask is 0)
                        {
                            const uint32_t lm = acc & ~unlisted;
                            if ((acc & unlisted) != 0u && (lm & (lm - 1u)) == 0u) depth |= acc << kDirectShift;
                        }
                    }
                }
            }
            if (term) stq(&wf.radiance[pid], make_float4(L.x, L.y, L.z, 0.0f));   // (kNoRay slots: 0)
        }
        ndirect += (uint32_t)__popcll(__ballot(direct));        // (wave-uniform: a scalar register)
        // next ray: the wave's continuing lanes take consecutive slots of queue b+1
        const uint64_t m = __ballot(cont);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            uint32_t b0 = 0;
            if (lane == leader) b0 = atomicAdd(&lnext, (uint32_t)__popcll(m));
            b0 = lane_bcast(b0, leader);
            if (cont) {
                const size_t ji = seg0 + b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                stq(&qb2[qf(ji, kQO, qs)], pack(o, pid));
                stq(&qb2[qf(ji, kQD, qs)], pack(d, depth + 1u));
                stq(&qb2[qf(ji, kQPS, qs)], pack(color, sd));
            }
        }
        // carry: the resolved ray stays in this lane, as the words the tail would hold, and
        // enters the shading code above with its hit id in the wave's next iteration --
        // neither written nor read back; at most kCarryMax times in a row
        if constexpr (!SORTB) {
            carry = wf.shade_cull && rhit >= 0 && (kCarryMax == ~0u || nchain < kCarryMax);
            if constexpr (kCarryMax != ~0u) nchain = carry ? nchain + 1u : 0u;
        }
        // resolved rays that are not carried: the wave's take 64 consecutive slots from the
        // segment's last one downward, lanes ascending inside them, with their hit ids (head
        // and tail together hold at most this queue's rays, <= seg: they never meet)
        const bool totail = rhit >= 0 && !carry;
        const uint64_t mr = __ballot(totail);
        if (mr) {
            const int leader = __ffsll((unsigned long long)mr) - 1;
            const uint32_t nr = (uint32_t)__popcll(mr);
            uint32_t t0 = 0;
            if (lane == leader) t0 = atomicAdd(&ltail, nr);
            t0 = lane_bcast(t0, leader);
            if (totail) {
                const size_t ji = seg0 + (wf.seg - t0 - nr) + (uint32_t)__popcll(mr & ((1ull << lane) - 1ull));
                stq(&qb2[qf(ji, kQO, qs)], pack(o, pid));
                stq(&qb2[qf(ji, kQD, qs)], pack(d, depth + 1u));
                stq(&qb2[qf(ji, kQPS, qs)], pack(color, sd));
                reinterpret_cast<int32_t*>(qb2 + qf(0, kQHIT, qs))[ji] = rhit;
            }
        }
