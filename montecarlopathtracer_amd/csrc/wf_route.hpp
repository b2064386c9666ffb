// wf_route.hpp -- the route of a wavefront render: which of the pipeline's
// steps run and with how much LDS, decided once per render from facts about the
// scene and the render, and the batch split.  Host code only (plain C++ over
// render_launch.hpp): plan.cpp computes the route (make_plan; a listed pass
// again in prepare_wavefront_list), it travels in Plan, and the workspace layout,
// mcpt_plan_query, mcpt_scene_primary_shade_lds and launch_wavefront read it.
// The features' own descriptions are render_launch.hpp's.
#pragma once

#include "render_launch.hpp"

// The build flags the route reads (wf_device.hpp has the others, and includes
// this header).
// Bounce 0 of CV mode by the wave-coherent packet extend (wavefront_primary.hip)
#ifndef MCPT_WF_PACKET0
#define MCPT_WF_PACKET0 1
#endif
// MCPT_WF_GEN0 (default 1): no generate kernel before the packet extend -- each
// lane computes its slot's primary ray itself (the inverse dealing slot_pid
// and primary_ray, as bounce 0's shade already does), writes the segment's
// queue length and counts the paths; queue 0 holds no direction stream.
// Generate was the only kernel of a frame's start (0.9 ms of one rank's 33 ms
// share at N = 8) and moved 16 B per path through HBM twice.
#ifndef MCPT_WF_GEN0
#define MCPT_WF_GEN0 1
#endif
// MCPT_WF_IMPLICIT0 = 1: bounce 0's shade (queue order, CV mode) recomputes a
// primary ray's origin, direction and RNG state from its slot instead of
// reading them, and generate skips the {throughput, rng} stream (64 B of
// queue traffic less per path); 2 (default): also the {o, pid} stream
// (extend's bounce-0 origins are the eye; 32 B more).  With MCPT_WF_NT = 3:
// level 1 C2 wavefront +0.3%, level 2 +0.9% (C4 +1.4%).
#ifndef MCPT_WF_IMPLICIT0
#define MCPT_WF_IMPLICIT0 2
#endif
// (measurements: wf_device.hpp "Residency of the global-memory extend" and below it)
#ifndef MCPT_WF_GLOBAL_S
#define MCPT_WF_GLOBAL_S 6
#endif
#ifndef MCPT_WF_SHADE_LDS_BLOCK
#define MCPT_WF_SHADE_LDS_BLOCK 512
#endif
#ifndef MCPT_WF_GEO_LDS
#define MCPT_WF_GEO_LDS 1
#endif

namespace mcpt {

constexpr size_t kLdsPerCu = 160 * 1024;
// the shade's static LDS: its copy of the direct lists' records and 64 B of counters
constexpr size_t kShadeStaticLds = kDirectShadeLds + 64;

// direct lists: the lean LDS extend keeps its table (a clipped ray's listed box)
// behind the counter block, and the shade's static LDS must fit beside the
// extend's workgroup.  Neither decides where a scene lives: if they do not fit
// beside the image the scene stays in LDS and its renders make no direct rays
// and no selectors
inline bool direct_lists_fit(uint32_t image_bytes, uint32_t node_boxes) {
    return !node_boxes && lds_bytes_counted_in_lds(image_bytes, 4) + kShadeStaticLds + kDirectLdsBytes <= kMaxLds;
}

// What the route is computed from.  The scene: its GpuScene and what its
// route tables hold for the culls (n_cull_boxes as far as the render may use
// them: plan.cpp plan_route).  The render: its parameters as make_plan read them
struct WfFacts {
    const GpuScene* scene;
    uint32_t n_miss_boxes, direct_counts, n_cull_boxes;
    int cus;
    bool lean, sort, qe;
    bool listed;                         // a frame with an explicit queue 0: over a pixel list
                                         // (KernelParams::pixel_list) or over ray buffers (a ray frame)
    bool default_batch;                  // the plan chose the batch (mcpt_render_params::wf_batch 0)
    bool tile_records;                   // the workspace has the primary lists' tile records (wf_layout)
    int tile, max_depth;
    uint32_t group_shift;                // the plan's, for a scene in global memory
    // sphere clip: the scene's mask and spheres (RouteTables::clip_spheres, ::clip_sphere; null: none)
    uint32_t clip_spheres;
    const float (*clip_sphere)[4];
};

struct WfRoute {
    int cus;
    bool in_lds;                         // scene_in_lds
    uint32_t nseg;                       // queue segments = extend workgroups
    int variant;                         // mcpt_render_stats::variant: 4 in LDS, 5 in global memory
    int queries;                         // extends of a path: max_depth + 1, QuinEngine 3 * max_depth + 1
    int terminal;                        // the last query's depth
    uint32_t n_miss_boxes;               // miss cull: the scene's boxes, lean renders only
    uint32_t direct_counts;              // direct lists: the scene's counts where the lists are active, else 0
    uint32_t n_cull_boxes;               // terminal cull: the boxes the render may use
    bool direct;                         // the direct lists are active (direct resolve, clip walk)
    bool shade_cull;                     // the queue-order shade owns the terminal cull (WfParams::shade_cull)
    bool carry;                          // ... and carries the rays it resolves: the schedule's question
    bool packet;                         // bounce 0 by the packet extend
    bool generate;                       // a generate kernel fills queue 0
    bool can_list;                       // bounce 0 may read the primary lists (a batch of whole tiles does)
    bool whole;                          // the batch split keeps whole 8x8 tiles
    bool primary_shade;                  // a batch that reads the lists also shades bounce 0 (wf_primary_shade)
    int cull_bounce;                     // wf_cull_terminal runs on this bounce's queue; -1: not at all
    uint32_t group_shift, xcd_deal;      // WfParams' dealing of paths to segments
    // dynamic LDS of a workgroup: the packet extend and its list form; the
    // extend (with the direct table where the lists are active: direct_lds);
    // wf_primary_shade; the shade's material table (0: read from global memory)
    size_t packet_lds, extend_lds, direct_lds, primary_shade_lds, geo_lds;
    // sphere clip: the scene's spheres where the secondary extends are wf_sphere_clip, else mask 0
    SphereClip clip;
};

inline WfRoute wf_route(const WfFacts& f) {
    const GpuScene& sc = *f.scene;
    WfRoute r{};
    r.cus = f.cus;
    r.in_lds = scene_in_lds(sc);
    r.nseg = uint32_t(f.cus) * (r.in_lds ? 1u : uint32_t(kWfGlobalSegsPerCu));
    r.variant = r.in_lds ? 4 : 5;
    // a ray's depth is at most 3 * max_depth + 1 (QuinEngine)
    r.queries = (f.qe ? 3 : 1) * f.max_depth + 1;
    r.terminal = r.queries - 1;
    // (counting renders walk every ray: their visit counters stay the oracle's)
    r.n_miss_boxes = f.lean ? f.n_miss_boxes : 0u;
    // direct lists: active where the miss cull runs in front of the lean LDS
    // extend and the tables fit beside the image (which implies a scene in LDS)
    r.direct = r.n_miss_boxes && f.direct_counts && direct_lists_fit(sc.image_bytes, sc.node_boxes);
    r.direct_counts = r.direct ? f.direct_counts : 0u;
    r.n_cull_boxes = f.n_cull_boxes;
    // the queue-order shade of a lean render of an LDS scene with occluder boxes
    // culls the terminal query's rays where it makes them and carries the rays it
    // resolves; queues then hold mixed depths, and no wf_cull_terminal runs
    r.shade_cull = f.lean && r.in_lds && !f.sort && r.n_miss_boxes != 0;
    r.carry = r.shade_cull && r.direct;
    // sphere clip: where the lean LDS extend clips walks (the lists active, the
    // queue-order shade, CV mode) and a box without a list has a sphere, the
    // secondary extends also cut a clipped ray's walk to its boxes' spheres
    if (r.direct && f.lean && r.in_lds && !f.sort && !f.qe && f.clip_sphere) {
        r.clip.mask = f.clip_spheres;
        for (int b = 0; b < kMaxMissBoxes; b++)
            for (int a = 0; a < 4; a++) r.clip.sphere[b][a] = f.clip_sphere[b][a];
    }
    // LDS scenes: one 8x8 tile of one sample per group; global-memory scenes:
    // the planned group size (whole image regions per segment), dealt by XCD (seg_of)
    r.group_shift = r.in_lds ? 6u : f.group_shift;
    r.xcd_deal = r.in_lds ? 0u : 1u;
    // bounce 0 of CV mode with an implicit queue 0 (every origin is the eye; not a
    // listed frame, whose slots do not name their pixels): the wave-coherent
    // extend, one tree walk per 64-ray tile, which also generates the primary rays
    // (the packet extend stores hit ids only: it needs the queue-order shade)
    r.packet = MCPT_WF_PACKET0 && MCPT_WF_IMPLICIT0 >= 2 && r.in_lds && !f.qe && !f.listed;
    r.generate = !(r.packet && MCPT_WF_GEN0);
    // primary lists: lean renders where the packet extend runs whose tiles are
    // 8x8 -- one tile of one sample per 64-slot group -- and whose scene a
    // per-tile scan of every triangle suits (kListMaxTris)
    r.can_list = r.packet && MCPT_WF_GEN0 && f.lean && f.tile == 8 && sc.n_tris <= kListMaxTris && f.tile_records;
    // (a batch size the caller asked for is kept as asked)
    r.whole = r.can_list && f.default_batch;
    // primary shade: where the queue-order shade culls and carries, the kernel that
    // resolves the groups also shades them and fills queue 1 -- no bounce-0 shade
    r.primary_shade = r.can_list && r.shade_cull;
    // the terminal query's queue (CV: a scene with emitter boxes; QE: every ray)
    // loses the rays whose hit adds nothing, behind the shade that fills it;
    // counting renders keep the full walk, and where the shade culls such a ray as
    // it makes it none is left
    r.cull_bounce = (f.lean && !r.shade_cull && r.terminal >= 1 && (f.qe || f.n_cull_boxes)) ? r.terminal : -1;
    r.packet_lds = r.in_lds ? lds_bytes_counted_in_lds(sc.image_bytes, 4) : 0;
    r.direct_lds = r.direct ? kDirectLdsBytes : 0;
    r.extend_lds = r.in_lds ? r.packet_lds + r.direct_lds : lds_bytes_global(MCPT_WF_GLOBAL_S, true);
    // (the lean LDS extend's -- stack, image, counter block -- and its table; no static LDS)
    r.primary_shade_lds = r.in_lds ? r.packet_lds + r.direct_lds : 0;
    // the shade's material table in LDS if it fits beside the extend's workgroups on a CU
    const size_t ext_cu = r.in_lds ? r.extend_lds : kWfGlobalSegsPerCu * r.extend_lds;
    const size_t geo = 64 * size_t(sc.n_geoms);
    r.geo_lds = (MCPT_WF_GEO_LDS && ext_cu + kShadeStaticLds + geo <= kLdsPerCu) ? geo : 0;
    return r;
}

// The shade's workgroup: alone on the GPU (one stream) 16 waves per segment
// keep HBM busy; beside an LDS extend workgroup 8 waves (2 x 80 VGPRs per
// SIMD); 256 threads beside the global-memory extend's four workgroups
inline int wf_shade_block(const WfRoute& r, int streams) {
    return r.in_lds ? (streams == 1 ? 1024 : MCPT_WF_SHADE_LDS_BLOCK) : 256;
}

// The batch split of a render, one run of chunks at a time: from `chunk` on,
// ncb chunks of nsc samples each are rendered together (whole-image batches may
// span several full chunks: fewer, longer launches), in batches of at most
// nb_max pixels each.  whole: batches that cut the frame hold whole 8x8 tiles
// (a default batch of a render that can use the primary lists: work / streams
// pixels are no whole tiles when the tile count is odd, nor is a batch over a
// chunk length that does not divide it, and such a render would walk every
// primary ray).
struct WfSpan {
    uint32_t nsc, ncb, nb_max;
};
inline WfSpan wf_span(const KernelParams& kp, uint32_t capacity, uint32_t chunk, bool whole) {
    WfSpan s;
    s.nsc = (kp.spp - chunk * kp.chunk) < kp.chunk ? (kp.spp - chunk * kp.chunk) : kp.chunk;
    s.ncb = 1;
    if (s.nsc == kp.chunk && (uint64_t)kp.npix_local * kp.chunk <= capacity) {
        const uint32_t full = (kp.spp / kp.chunk) - chunk;             // full chunks left
        const uint32_t fit = (uint32_t)(capacity / ((uint64_t)kp.npix_local * kp.chunk));
        s.ncb = fit < full ? fit : full;
    }
    s.nb_max = capacity / (s.ncb * s.nsc);
    if (whole && s.nb_max >= 64u && s.nb_max < kp.npix_local) s.nb_max &= ~63u;
    return s;
}
// every batch of the split in launch order: fn(span, first chunk, first pixel) -> false ends the walk
template <typename F>
void wf_for_each_batch(const KernelParams& kp, uint32_t capacity, bool whole, F&& fn) {
    for (uint32_t chunk = 0; chunk < kp.nchunks;) {
        const WfSpan s = wf_span(kp, capacity, chunk, whole);
        for (uint32_t v0 = 0; v0 < kp.npix_local; v0 += s.nb_max)
            if (!fn(s, chunk, v0)) return;
        chunk += s.ncb;
    }
}
// The per-batch fields of a stream's WfParams (everything else the plan
// filled, plan.cpp prepare_wavefront): pixels [v0, v0 + nb_max) of the frame x
// the span's chunks from chunk0 on
inline WfParams wf_batch_params(const WfParams& of_stream, const WfRoute& r, const KernelParams& kp, const WfSpan& span,
                                uint32_t chunk0, uint32_t v0) {
    WfParams wf = of_stream;
    wf.chunk_index = chunk0;
    wf.s_begin = chunk0 * kp.chunk;
    wf.nsc = span.nsc;
    wf.ns = span.ncb * span.nsc;
    wf.v0 = v0;
    wf.nb = (kp.npix_local - v0) < span.nb_max ? (kp.npix_local - v0) : span.nb_max;
    const uint32_t n = wf.nb * wf.ns;
    // whole groups per segment
    wf.seg = ((((n + (1u << r.group_shift) - 1u) >> r.group_shift) + r.nseg - 1) / r.nseg) << r.group_shift;
    return wf;
}
// (a batch whose pixel range is not whole 8x8 tiles keeps the walk: its 64-slot
// groups would straddle tiles)
inline bool whole_tiles(uint32_t v0, uint32_t nb) { return (v0 & 63u) == 0u && (nb & 63u) == 0u; }
// whether any batch of the split is whole tiles, i.e. can read the primary lists
inline bool any_whole_tile_batch(const KernelParams& kp, uint32_t capacity, bool whole) {
    for (uint32_t chunk = 0; chunk < kp.nchunks;) {
        const WfSpan s = wf_span(kp, capacity, chunk, whole);
        chunk += s.ncb;
        // every batch but the last holds nb_max pixels: whole tiles only if nb_max is (then
        // all are; npix_local is whole 8x8 tiles); else the last one alone can be, which
        // ends with the frame, if it starts on a tile
        const uint32_t last_v0 = (kp.npix_local - 1u) / s.nb_max * s.nb_max;
        if ((s.nb_max & 63u) == 0u || whole_tiles(last_v0, kp.npix_local - last_v0)) return true;
    }
    return false;
}

}  // namespace mcpt
