// wf_primary_pairs.hpp -- a listed group's resolve (render_launch.hpp "Primary
// lists"): the tile's up to kListK candidate triangles tested two at a time from
// their LDS records, the next pair's indices loaded behind the current pair's
// tests.  Included as source text by wf_primary_body.hpp (wf_primary_lists) and
// by wf_primary_shade_body.hpp (wf_primary_shade): one statement of how a
// record is read.  In scope: tris, ncand, h4 (the record's first four words),
// rec (the record); per lane: the ray r (begin_ray done where active), active.
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
