// wf_primary_walk.hpp -- the packet walk of one 64-ray group (wavefront_primary.hip's
// header comment says how it works), included as source text by
// wf_primary_body.hpp (wf_extend_primary, wf_primary_lists) and by
// wf_primary_shade_body.hpp (wf_primary_shade): one copy of the walk, and the
// first two kernels' code stays what it was.  In scope: S, BLOCK, COUNT, U, sc,
// eye, tris, nodes, leafs, st, spill, spill_stride, c; per lane: the ray r
// (begin_ray done where active), active, done.  On leaving, r holds each lane's
// closest hit.
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
