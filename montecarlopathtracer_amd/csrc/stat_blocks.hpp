// stat_blocks.hpp -- the small device blocks the kernels count into and the host
// reads back: a render's (Workspace::small) and the ray queries' (mcpt_scene::rq_stats).
// Plain C++ over <stdint.h>: kernels, host code and host probes share one layout.
// A new counter is a new enumerator in front of kStatSlots and nothing else.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mcpt {

// the slots of KernelParams::stats
enum StatSlot : int {
    // the eight Counters, in flush_counters' order (trace_device.hpp); mcpt_render_stats'
    // fields of the same names (stats_from_counters)
    kStatRays = 0,
    kStatPaths,
    kStatInnerVisits,
    kStatLeafVisits,
    kStatLeafRefs,
    kStatTriTests,
    kStatShades,
    kStatStackSpills,
    kStatCounters,                       // (their number)
    // diagnostic builds (-DMCPT_PHASE_TIMING): cycles summed over waves, as the megakernel
    // names them; the wavefront extend counts setup, traversal bursts, hand-offs, burst
    // iterations and the number of hand-offs into the same five
    kStatPhaseUnits = kStatCounters,
    kStatPhaseTrav,
    kStatPhaseShade,
    kStatPhaseIters,
    kStatPhaseScatter,
    // the routes a wavefront render's rays took (render_launch.hpp has each feature's account)
    kStatDirect,                         // direct rays, counted by the shades that resolve them
    kStatExtend,                         // rays the secondary extends (bounce >= 1) took, one atomic per workgroup
    kStatClipped,                        // of those, the rays an extend started with a selector (clip walk)
    kStatPrimaryShaded,                  // paths whose bounce 0 wf_primary_shade shaded
    kStatSphereSkips,                    // selected rays whose walk a sphere left nothing of (wf_sphere_clip, per wave)
    kStatSlots
};
static_assert(kStatCounters == 8, "Counters has eight fields");

// A render's block.  counter: the work-unit counter the persistent kernels hand units
// out from, alone in its 64 bytes.  stats: read and cleared by every stats record
// (render_host.cpp read_stats).  tile_classes: the last render's primary lists {no
// candidate, 1..K, more} and a spare word, cleared by every render and never by a read
struct RenderBlock {
    uint32_t counter[16];
    unsigned long long stats[kStatSlots];
    uint32_t tile_classes[4];
};
static_assert(offsetof(RenderBlock, stats) == 64, "the work-unit counter keeps 64 bytes of its own");
static_assert(offsetof(RenderBlock, stats) % 8 == 0 && alignof(RenderBlock) >= 8, "64-bit atomics on the stats");

// The ray and radiance queries' counters (the eight Counters each): the device entries'
// block (mcpt_trace_stats_read reads and clears it) and the synchronous host entries'
struct QueryBlocks {
    unsigned long long device[kStatCounters], host[kStatCounters];
};
// A wavefront radiance query's block (mcpt_radiance_ex_device, mcpt_scene::rad_wf_stats).
// stats: the KernelParams::stats of the query's kernels -- all kStatSlots of them: the
// wavefront's shades and extends also add to the route slots behind the eight Counters,
// which a QueryBlocks member has no room for.  Cleared on the query's stream in front of
// it and folded behind it (wf_ray_fold_stats): the Counters into QueryBlocks::device or
// ::host, the routes of a device-entry query into `routes`, {direct, extend, clipped,
// sphere_skips}, which mcpt_trace_stats_read reads and clears with the device block
constexpr int kQueryRoutes = 4;
struct WfQueryBlock {
    unsigned long long stats[kStatSlots];
    unsigned long long routes[kQueryRoutes];
};
// a work-unit counter on its own (the radiance queries': mcpt_scene::rad_small)
constexpr size_t kUnitCounterBytes = sizeof(RenderBlock::counter);

}  // namespace mcpt
