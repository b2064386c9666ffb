// queries.cpp -- the ray entries of the C ABI (include/mcpt.h): closest-hit and
// any-hit queries over ray buffers (rayquery.hip), path-traced radiance over
// ray buffers (render.hip radiance_kernel; on the wavefront pipeline as a ray
// frame, wavefront_rays.hip), ambient occlusion of point buffers and of a frame's
// first hits (ao.hip), direct lighting of the same by area sampling of the scene's
// light table (direct.hip), and mcpt_intersect on the older closest-hit kernel the
// ray-query tests compare against.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "ao_launch.hpp"
#include "capi_internal.hpp"
#include "direct_launch.hpp"
#include "rayquery_launch.hpp"

using namespace mcpt::host;

namespace {

// ---- device ray queries (rayquery.hip) ----------------------------------------
// The checks of a ray query that need no device, in the header's order; p
// resolved (NULL = the defaults).  `closest`: mcpt_trace_device (kind is read).
mcpt_trace_params trace_resolve(const mcpt_scene* s, const mcpt_trace_params* p, int64_t n, bool ptrs, bool closest) {
    if (!s) throw mcpt::Error{MCPT_E_INVALID, "NULL scene"};
    if (n < 0) throw mcpt::Error{MCPT_E_INVALID, "n must be >= 0"};
    if (n && !ptrs) throw mcpt::Error{MCPT_E_INVALID, "NULL ray or result buffer"};
    mcpt_trace_params q;
    mcpt_trace_params_default(&q);
    if (p) q = *p;
    if (closest && q.kind != MCPT_TRACE_CLOSEST && q.kind != MCPT_TRACE_ANY)
        throw mcpt::Error{MCPT_E_INVALID, "kind must be MCPT_TRACE_CLOSEST or MCPT_TRACE_ANY"};
    if (!(q.t_max >= 0.0f)) throw mcpt::Error{MCPT_E_INVALID, "t_max must be >= 0 (0 = FLT_MAX)"};
    if (q.lean != 0 && q.lean != 1) throw mcpt::Error{MCPT_E_INVALID, "lean must be 0 or 1"};
    if (q.workgroups < 0) throw mcpt::Error{MCPT_E_INVALID, "workgroups must be >= 0"};
    if (q.refill < 0 || q.refill > 64) throw mcpt::Error{MCPT_E_INVALID, "refill must be 0 (default) or 1..64"};
    if (n >= (int64_t(1) << 31) / 3) throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many rays for one call"};
    if (closest && q.kind == MCPT_TRACE_ANY)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "kind MCPT_TRACE_ANY reports a flag, not a triangle: "
                                              "call mcpt_occluded_device"};
    if (!s->on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    if (q.t_max == 0.0f) q.t_max = FLT_MAX;
    return q;
}

// What the ray queries need on the scene's (current) device: tri_order, the
// counter blocks and the renders' stack spill area.  Nothing once they exist.
void ensure_rays(mcpt_scene& s, bool capturing) {
    if (capturing && (!s.rq_order.p || !s.rq_stats.p))
        throw mcpt::Error{MCPT_E_NOMEM, "the first ray query of a scene allocates: call mcpt_scene_reserve_rays "
                                        "before capturing a graph"};
    grow_spill(s, 1, capturing);
    if (!s.rq_order.p) {
        const size_t bytes = s.tri_order.size() * 4;
        TempDev t(bytes);
        if (bytes) HIP_TRY(hipMemcpy(t.p, s.tri_order.data(), bytes, hipMemcpyHostToDevice));
        s.rq_order.p = t.release();
    }
    if (!s.rq_stats.p) {
        TempDev t(sizeof(mcpt::QueryBlocks));
        HIP_TRY(hipMemset(t.p, 0, sizeof(mcpt::QueryBlocks)));
        HIP_TRY(mcpt::prepare_rayquery(s.gpu));   // (the kernels' code object loaded now)
        s.rq_stats.p = t.release();
    }
}

// One query on st: closest hit (d_occ NULL) or any hit.  host_block: count
// into the host entry's counter block.
void rays_async(mcpt_scene& s, const mcpt_trace_params& q, int64_t n, const float* d_o, const float* d_d,
                const float* d_t_max, int32_t* d_tri, float* d_hit, uint8_t* d_occ, bool host_block, hipStream_t st) {
    ensure_rays(s, stream_capturing(st));
    mcpt::RayQueryParams rq{};
    rq.scene = s.gpu;
    rq.o = d_o;
    rq.d = d_d;
    rq.t_max = d_t_max;
    rq.tri = d_tri;
    rq.hit = d_hit;
    rq.occ = d_occ;
    rq.tri_order = static_cast<const uint32_t*>(s.rq_order.p);
    rq.spill = static_cast<uint4*>(s.ws.spill.p);
    rq.spill_stride = static_cast<uint32_t>(launched_lanes(s));
    rq.stats = host_block ? query_blocks(s)->host : query_blocks(s)->device;
    rq.n = static_cast<uint32_t>(n);
    rq.refill = q.refill;
    rq.best_init = q.t_max;
    HIP_TRY(mcpt::launch_rayquery(rq, d_occ != nullptr, q.lean != 0, s.cus, q.workgroups, st));
}

// ---- device radiance queries (render.hip radiance_kernel) -----------------------
struct Radiance {
    mcpt_radiance_params q;
    uint32_t chunk;
    uint64_t nchunks;
};
// The checks of a radiance query that need no device, in the header's order, up to
// the work-unit limit; p resolved (NULL = the defaults)
Radiance radiance_checks(const mcpt_scene* s, const mcpt_radiance_params* p, int64_t n, bool ptrs) {
    if (!s) throw mcpt::Error{MCPT_E_INVALID, "NULL scene"};
    if (n < 0) throw mcpt::Error{MCPT_E_INVALID, "n must be >= 0"};
    if (n && !ptrs) throw mcpt::Error{MCPT_E_INVALID, "NULL ray or result buffer"};
    Radiance R;
    mcpt_radiance_params& q = R.q;
    mcpt_radiance_params_default(&q);
    if (p) q = *p;
    if (q.spp == 0) throw mcpt::Error{MCPT_E_INVALID, "spp must be >= 1"};
    if (q.max_depth < 0 || q.max_depth > mcpt::kMaxDepthParam)
        throw mcpt::Error{MCPT_E_INVALID, "max_depth must be 0..1000"};
    if (!std::isfinite(q.illum)) throw mcpt::Error{MCPT_E_INVALID, "illum must be finite"};
    if (q.lean != 0 && q.lean != 1) throw mcpt::Error{MCPT_E_INVALID, "lean must be 0 or 1"};
    if (q.fresnel_kd != 0 && q.fresnel_kd != 1) throw mcpt::Error{MCPT_E_INVALID, "fresnel_kd must be 0 or 1"};
    if (q.workgroups < 0) throw mcpt::Error{MCPT_E_INVALID, "workgroups must be >= 0"};
    if (q.ready_thresh < 0 || q.ready_thresh > 64)
        throw mcpt::Error{MCPT_E_INVALID, "ready_thresh must be 0 (default) or 1..64"};
    if (uint64_t(q.spp_offset) + uint64_t(q.spp) > (uint64_t(1) << 32))
        throw mcpt::Error{MCPT_E_INVALID, "spp_offset + spp must not pass 2^32"};
    R.chunk = q.spp_chunk ? (q.spp_chunk < q.spp ? q.spp_chunk : q.spp) : q.spp;
    R.nchunks = (uint64_t(q.spp) + R.chunk - 1) / R.chunk;
    if (n >= (int64_t(1) << 31) / 3) throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many rays for one call"};
    if (uint64_t(n) * R.nchunks >= (uint64_t(1) << 31))
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many work units (rays x chunks) for one call"};
    return R;
}
// ... and the host-only scene behind them
Radiance radiance_resolve(const mcpt_scene* s, const mcpt_radiance_params* p, int64_t n, bool ptrs) {
    const Radiance R = radiance_checks(s, p, n, ptrs);
    if (!s->on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    return R;
}
// A query with its pipeline (mcpt_radiance_ex*): mcpt_radiance's checks, then the
// wavefront fields with mcpt_render_params' ranges and messages (plan.cpp make_plan),
// then the host-only scene; x resolved (NULL = the defaults, the megakernel)
struct RadianceEx {
    Radiance R;
    mcpt_radiance_ex_params x;
    bool wavefront() const { return x.pipeline == MCPT_PIPELINE_WAVEFRONT; }
};
RadianceEx radiance_ex_resolve(const mcpt_scene* s, const mcpt_radiance_ex_params* p, int64_t n, bool ptrs) {
    RadianceEx E;
    mcpt_radiance_ex_params_default(&E.x);
    if (p) E.x = *p;
    E.R = radiance_checks(s, &E.x.base, n, ptrs);
    const mcpt_radiance_ex_params& x = E.x;
    if (x.pipeline != MCPT_PIPELINE_MEGAKERNEL && x.pipeline != MCPT_PIPELINE_WAVEFRONT)
        throw mcpt::Error{MCPT_E_INVALID, "unknown pipeline"};
    if (x.wf_streams < 0 || x.wf_streams > mcpt::kMaxWfStreams)
        throw mcpt::Error{MCPT_E_INVALID, "wf_streams must be 0 (automatic) or 1..4"};
    if (x.wf_refill < 0 || x.wf_refill > 64)
        throw mcpt::Error{MCPT_E_INVALID, "wf_refill / ready_thresh must be 0 (automatic) or 1..64"};
    if (x.wf_group_shift != 0 && (x.wf_group_shift < 6 || x.wf_group_shift > 14))
        throw mcpt::Error{MCPT_E_INVALID, "wf_group_shift must be 0 (automatic) or 6..14"};
    if (!s->on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    return E;
}

// The kernel parameters of a query: a packed frame of n rays (no pixel decode
// is run), its chunks, and the tail split of the megakernel -- the last units
// per lane handed out one sample at a time; the workspace pointers come later
mcpt::KernelParams radiance_plan(const mcpt_scene& s, const Radiance& R, int64_t n, uint64_t* tail_out) {
    const mcpt_radiance_params& q = R.q;
    mcpt::KernelParams k;
    std::memset(&k, 0, sizeof k);
    k.scene = s.gpu;
    k.width = static_cast<int32_t>(n); k.height = 1;
    k.tile = 1; k.tiles_x = static_cast<int32_t>(std::max<int64_t>(n, 1));
    k.shard_count = 1; k.packed = 1;
    k.npix_local = static_cast<uint32_t>(n);
    k.spp = q.spp; k.spp_offset = q.spp_offset; k.chunk = R.chunk;
    k.nchunks = static_cast<uint32_t>(R.nchunks);
    k.total_units = static_cast<uint32_t>(uint64_t(n) * R.nchunks);
    k.div_npix = mcpt::FastDiv::make(std::max<uint32_t>(k.npix_local, 1));
    k.div_tt = mcpt::FastDiv::make(1);
    k.div_tiles_x = mcpt::FastDiv::make(static_cast<uint32_t>(k.tiles_x));
    k.div_tile = mcpt::FastDiv::make(1);
    k.div_chunk = mcpt::FastDiv::make(R.chunk);
    k.max_depth = q.max_depth;
    k.lean = q.lean;
    k.illum = q.illum;
    k.fresnel_kd = q.fresnel_kd;
    k.prev_count = q.prev_count;
    k.mode = MCPT_MODE_CVMCTRACER;
    k.best_init = FLT_MAX;
    k.key = tea16(static_cast<uint32_t>(q.seed), static_cast<uint32_t>(q.seed >> 32));
    k.ready_thresh = ready_thresh_for(s, q.ready_thresh);
    // the renders' tail split at its default units per lane
    const uint64_t tail = tail_split(launched_lanes(s), kTailPerLane, 0, k.total_units, k.chunk);
    k.tail_units = k.total_units - static_cast<uint32_t>(tail);
    k.total_items = k.tail_units + static_cast<uint32_t>(tail * k.chunk);
    *tail_out = tail;
    return k;
}

// The query's workspace on the scene's (current) device, grown to what k needs:
// the ray queries' counter blocks and the renders' spill area (ensure_rays),
// the partial sums, the tail samples, the work-unit counter
void ensure_radiance(mcpt_scene& s, mcpt::KernelParams& k, uint64_t tail, bool host_block, bool capturing) {
    if (capturing && (!s.rq_order.p || !s.rq_stats.p || !s.rad_small.p))
        throw mcpt::Error{MCPT_E_NOMEM, "the first radiance query of a scene allocates: call "
                                        "mcpt_scene_reserve_radiance before capturing a graph"};
    ensure_rays(s, capturing);
    if (!s.rad_small.p) {
        TempDev t(mcpt::kUnitCounterBytes);
        HIP_TRY(hipMemset(t.p, 0, mcpt::kUnitCounterBytes));
        HIP_TRY(mcpt::prepare_radiance(s.gpu));   // (the kernels' code object loaded now)
        s.rad_small.p = t.release();
    }
    grow_ws(s, s.rad_partial, size_t(k.total_units) * 16, capturing);
    if (tail) grow_ws(s, s.rad_tail, size_t(tail) * k.chunk * 16, capturing);
    k.partial = static_cast<float4*>(s.rad_partial.p);
    k.tail_buf = tail ? static_cast<float4*>(s.rad_tail.p) : nullptr;
    k.counter = static_cast<uint32_t*>(s.rad_small.p);
    k.stats = host_block ? query_blocks(s)->host : query_blocks(s)->device;
    k.spill = static_cast<uint4*>(s.ws.spill.p);
}

void radiance_async(mcpt_scene& s, const Radiance& R, int64_t n, const float* d_o, const float* d_d,
                    const uint32_t* d_stream, float* d_out, bool host_block, hipStream_t st) {
    uint64_t tail = 0;
    mcpt::KernelParams k = radiance_plan(s, R, n, &tail);
    ensure_radiance(s, k, tail, host_block, stream_capturing(st));
    const mcpt::RayInputs ri{d_o, d_d, d_stream};
    HIP_TRY(mcpt::launch_radiance(k, ri, s.cus, R.q.workgroups, reinterpret_cast<float4*>(d_out), st));
}

// ---- the wavefront form (wavefront_rays.hip, render_launch.hpp "Ray frames") ------
// What a wavefront query of n rays needs on the scene's (current) device, in place:
// the queries' counter blocks and its own, and the ray frame planned inside the
// scene's wavefront workspace (plan.cpp prepare_wavefront_rays).  The query and
// mcpt_scene_reserve_radiance_ex both run it, so the two agree
void prepare_radiance_wf(mcpt_scene& s, const RadianceEx& E, int64_t n, bool capturing, Prepared& P) {
    if (capturing && (!s.rq_order.p || !s.rq_stats.p || !s.rad_wf_stats.p))
        throw mcpt::Error{MCPT_E_NOMEM, "the first wavefront radiance query of a scene allocates: call "
                                        "mcpt_scene_reserve_radiance_ex before capturing a graph"};
    ensure_rays(s, capturing);
    if (!s.rad_wf_stats.p) {
        TempDev t(sizeof(mcpt::WfQueryBlock));
        HIP_TRY(hipMemset(t.p, 0, sizeof(mcpt::WfQueryBlock)));
        HIP_TRY(hipStreamSynchronize(nullptr));   // (as prepare_workspace: before a query on a non-blocking stream)
        s.rad_wf_stats.p = t.release();
    }
    uint64_t tail = 0;                    // (the megakernel's split: a ray frame has none)
    const mcpt::KernelParams k = radiance_plan(s, E.R, n, &tail);
    // the render parameters the wavefront's plan reads: the query's samples and its wavefront fields
    mcpt_render_params rp;
    mcpt_render_params_default(&rp);
    rp.pipeline = MCPT_PIPELINE_WAVEFRONT;
    rp.spp = E.R.q.spp;
    rp.wf_batch = E.x.wf_batch;
    rp.wf_streams = E.x.wf_streams;
    rp.wf_refill = E.x.wf_refill;
    rp.wf_group_shift = E.x.wf_group_shift;
    rp.wf_sort = E.x.wf_sort;
    rp.wf_mem_limit = E.x.wf_mem_limit;
    prepare_wavefront_rays(s, k, &rp, capturing, P);
}

// One wavefront query on st; returns the route's variant (4 in LDS, 5 in global memory).
// The kernels count into the query's own block of kStatSlots words -- the shades and
// extends also add to the route slots behind the eight Counters, which would overrun a
// QueryBlocks member -- cleared on st in front of them and folded on st behind the join
int radiance_wf_async(mcpt_scene& s, const RadianceEx& E, int64_t n, const float* d_o, const float* d_d,
                      const uint32_t* d_stream, float* d_out, bool host_block, hipStream_t st) {
    Prepared P;
    prepare_radiance_wf(s, E, n, stream_capturing(st), P);
    mcpt::WfQueryBlock* blk = wf_query_block(s);
    mcpt::KernelParams& k = P.pl.kp;
    k.stats = blk->stats;
    // "queue 0 is explicit" (implicit0): a valid device address that no kernel of a ray frame reads
    k.pixel_list = reinterpret_cast<const uint32_t*>(blk);
    HIP_TRY(hipMemsetAsync(blk->stats, 0, sizeof blk->stats, st));
    const mcpt::RayInputs ri{d_o, d_d, d_stream};
    int variant = 0;
    HIP_TRY(mcpt::launch_wavefront(k, P.pl.route, P.wf, wf_streams_on(s, P.pl.sets(), st), nullptr, nullptr, nullptr,
                                   reinterpret_cast<float4*>(d_out), &variant, &ri));
    HIP_TRY(mcpt::launch_wavefront_ray_fold(blk->stats, host_block ? query_blocks(s)->host : query_blocks(s)->device,
                                            host_block ? nullptr : blk->routes, st));
    return variant;
}

// the synchronous host entries' counter block (behind the device entries'), cleared
unsigned long long* clear_host_block(mcpt_scene& s) {
    unsigned long long* blk = query_blocks(s)->host;
    HIP_TRY(hipMemset(blk, 0, sizeof(mcpt::QueryBlocks::host)));
    return blk;
}

// The synchronous host entry of a radiance query (arguments checked): rays, stream ids
// and the result are staged in the scene's host-render buffer; run(d_o, d_d, d_stream,
// d_out) is the query on the null stream, counting into the host entries' block, and
// returns the record's variant
template <typename Run>
int radiance_host(mcpt_scene* s, const Radiance& R, int64_t n, const float* o, const float* d, const uint32_t* stream,
                  float* radiance, mcpt_render_stats* stats, Run&& run) {
    const size_t N = static_cast<size_t>(n);
    if (ranges_overlap(radiance, N * 12, o, N * 12) || ranges_overlap(radiance, N * 12, d, N * 12) ||
        ranges_overlap(radiance, N * 12, stream, stream ? N * 4 : 0))
        return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
    unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int variant = 0;
    if (n) {
        set_device(*s);
        const auto part = carve({N * 16, N * 12, N * 12, N * 4});
        ensure_buf(s->ws.fb, part.total);
        float* d_out = part.at<float>(s->ws.fb.p, 0);
        float* d_o = part.at<float>(s->ws.fb.p, 1);
        float* d_d = part.at<float>(s->ws.fb.p, 2);
        uint32_t* d_s = part.at<uint32_t>(s->ws.fb.p, 3);
        HIP_TRY(hipMemcpy(d_o, o, N * 12, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_d, d, N * 12, hipMemcpyHostToDevice));
        if (stream) HIP_TRY(hipMemcpy(d_s, stream, N * 4, hipMemcpyHostToDevice));
        std::vector<float> rgba(N * 4, 0.0f);
        if (R.q.prev_count) {
            rgb_to_rgba(radiance, N, rgba.data());
            HIP_TRY(hipMemcpy(d_out, rgba.data(), N * 16, hipMemcpyHostToDevice));
        }
        ensure_rays(*s, false);       // (the counter blocks exist before the host entry's is cleared)
        unsigned long long* blk = clear_host_block(*s);
        variant = run(d_o, d_d, stream ? d_s : nullptr, d_out);
        HIP_TRY(hipStreamSynchronize(nullptr));
        HIP_TRY(hipMemcpy(rgba.data(), d_out, N * 16, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c, blk, sizeof c, hipMemcpyDeviceToHost));
        rgba_to_rgb(rgba.data(), N, radiance);
    }
    if (stats) {
        stats_from_counters(c, *stats);
        stats->variant = variant;
    }
    return MCPT_OK;
}

// the device entry of a radiance query behind its parameter checks; wf: the wavefront form's query, or null
int radiance_device(mcpt_scene* s, const Radiance& R, const RadianceEx* wf, int64_t n, const float* d_o,
                    const float* d_d, const uint32_t* d_stream, float* d_radiance, void* hip_stream) {
    const size_t N = static_cast<size_t>(n);
    if (ranges_overlap(d_radiance, N * 16, d_o, N * 12) || ranges_overlap(d_radiance, N * 16, d_d, N * 12) ||
        ranges_overlap(d_radiance, N * 16, d_stream, d_stream ? N * 4 : 0))
        return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
    if (!n) return MCPT_OK;
    set_device(*s);                   // (a multi-device scene: devices[0], the primary)
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (wf) (void)radiance_wf_async(*s, *wf, n, d_o, d_d, d_stream, d_radiance, false, st);
    else radiance_async(*s, R, n, d_o, d_d, d_stream, d_radiance, false, st);
    return MCPT_OK;
}

// ---- ambient-occlusion queries (ao.hip) ------------------------------------------
// The checks of an AO query's own params, p resolved (NULL = the defaults) with its
// zeros for radius and bias replaced
mcpt_ao_params ao_fields(const mcpt_ao_params* p) {
    mcpt_ao_params q;
    mcpt_ao_params_default(&q);
    if (p) q = *p;
    if (q.spp == 0) throw mcpt::Error{MCPT_E_INVALID, "spp must be >= 1"};
    if (uint64_t(q.spp_offset) + uint64_t(q.spp) > (uint64_t(1) << 32))
        throw mcpt::Error{MCPT_E_INVALID, "spp_offset + spp must not pass 2^32"};
    if (!(q.radius >= 0.0f)) throw mcpt::Error{MCPT_E_INVALID, "radius must be >= 0 (0 = FLT_MAX)"};
    if (!(q.bias >= 0.0f) || !std::isfinite(q.bias))
        throw mcpt::Error{MCPT_E_INVALID, "bias must be > 0 and finite (0 = 0.01)"};
    if (q.lean != 0 && q.lean != 1) throw mcpt::Error{MCPT_E_INVALID, "lean must be 0 or 1"};
    if (q.workgroups < 0) throw mcpt::Error{MCPT_E_INVALID, "workgroups must be >= 0"};
    if (q.refill < 0 || q.refill > 64) throw mcpt::Error{MCPT_E_INVALID, "refill must be 0 (default) or 1..64"};
    if (q.unit_samples < 0) throw mcpt::Error{MCPT_E_INVALID, "unit_samples must be >= 0"};
    if (q.radius == 0.0f) q.radius = FLT_MAX;
    if (q.bias == 0.0f) q.bias = 0.01f;
    return q;
}
// The checks of the point form that need no device, in the header's order
mcpt_ao_params ao_resolve(const mcpt_scene* s, const mcpt_ao_params* p, int64_t n, bool ptrs) {
    if (!s) throw mcpt::Error{MCPT_E_INVALID, "NULL scene"};
    if (n < 0) throw mcpt::Error{MCPT_E_INVALID, "n must be >= 0"};
    if (n && !ptrs) throw mcpt::Error{MCPT_E_INVALID, "NULL point, normal or result buffer"};
    const mcpt_ao_params q = ao_fields(p);
    if (n >= (int64_t(1) << 31) / 3) throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many points for one call"};
    if (!s->on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    return q;
}
// The checks of a pixel form (ambient occlusion, direct lighting), in the header's
// order: the frame's fields it reads, the query's own params (fields(): they throw;
// returns the query's lean flag and its chunks per pixel), what it does not offer
// (`what` names the query), the host-only scene.  Returns the frame resolved: what
// make_plan reads of it and no field the query ignores
struct FrameQuery {
    int32_t lean;
    uint64_t chunks;
};
template <typename Fields>
mcpt_render_params frame_resolve(const mcpt_scene* s, const mcpt_render_params* rp, bool ptr, const std::string& what,
                                 Fields&& fields) {
    if (!s) throw mcpt::Error{MCPT_E_INVALID, "NULL scene"};
    if (!rp) throw mcpt::Error{MCPT_E_INVALID, "render params is NULL"};
    if (!ptr) throw mcpt::Error{MCPT_E_INVALID, "NULL result buffer"};
    if (rp->width <= 0 || rp->height <= 0) throw mcpt::Error{MCPT_E_INVALID, "width/height must be positive"};
    if (rp->spp == 0) throw mcpt::Error{MCPT_E_INVALID, "spp must be >= 1"};
    if (uint64_t(rp->spp_offset) + uint64_t(rp->spp) > (uint64_t(1) << 32))
        throw mcpt::Error{MCPT_E_INVALID, "spp_offset + spp must not pass 2^32"};
    if (rp->tile > 256) throw mcpt::Error{MCPT_E_INVALID, "tile too large"};
    if (rp->mode != MCPT_MODE_CVMCTRACER && rp->mode != MCPT_MODE_QUINENGINE)
        throw mcpt::Error{MCPT_E_INVALID, "unknown mode"};
    const FrameQuery fq = fields();
    const uint64_t T = rp->tile > 0 ? rp->tile : 8;
    const uint64_t padded = ((uint64_t(rp->width) + T - 1) / T) * ((uint64_t(rp->height) + T - 1) / T) * T * T;
    if (uint64_t(rp->width) * uint64_t(rp->height) >= (uint64_t(1) << 31) / 3 || padded >= (uint64_t(1) << 31))
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many pixels for one call"};
    if (padded * fq.chunks >= (uint64_t(1) << 31))
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many work units (pixels x chunks) for one call"};
    if (rp->mode == MCPT_MODE_QUINENGINE)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, what + " is not offered in QuinEngine mode"};
    if (rp->shard_count > 1 || rp->packed)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, what + " is not sharded: shard_count <= 1, packed = 0"};
    if (!s->on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    mcpt_render_params F;
    mcpt_render_params_default(&F);
    F.width = rp->width; F.height = rp->height;
    F.spp = rp->spp; F.spp_offset = rp->spp_offset;
    F.seed = rp->seed; F.prev_count = rp->prev_count;
    F.fov_deg = rp->fov_deg;
    for (int i = 0; i < 3; ++i) {
        F.eye[i] = rp->eye[i]; F.dir[i] = rp->dir[i]; F.up[i] = rp->up[i];
    }
    F.tile = rp->tile;
    F.max_depth = 0;
    F.lean = fq.lean;
    return F;
}
struct AoFrame {
    mcpt_render_params rp;
    mcpt_ao_params q;
};
AoFrame ao_frame_resolve(const mcpt_scene* s, const mcpt_render_params* rp, const mcpt_ao_params* ap, bool ptr) {
    AoFrame F;
    F.rp = frame_resolve(s, rp, ptr, "ambient occlusion", [&] {
        F.q = ao_fields(ap);
        return FrameQuery{F.q.lean, 1};
    });
    return F;
}

// What the AO queries need on the scene's (current) device for `points` points or
// pixels: the ray queries' (ensure_rays) and one count each.  Nothing once they exist.
void ensure_ao(mcpt_scene& s, uint64_t points, bool capturing) {
    if (capturing && (!s.rq_order.p || !s.rq_stats.p || !s.ao_counts.p))
        throw mcpt::Error{MCPT_E_NOMEM, "the first ambient-occlusion query of a scene allocates: call "
                                        "mcpt_scene_reserve_ao before capturing a graph"};
    ensure_rays(s, capturing);
    if (!s.ao_counts.p) HIP_TRY(mcpt::prepare_ao(s.gpu));   // (the kernels' code object loaded now)
    grow_ws(s, s.ao_counts, static_cast<size_t>(std::max<uint64_t>(points, 1)) * 4, capturing);
}

// One query on st over a filled a.kp (a.p, a.nrm, a.stream, a.out, a.points, a.out_n, a.pixel set)
void ao_async(mcpt_scene& s, const mcpt_ao_params& q, mcpt::AoParams& a, bool host_block, hipStream_t st) {
    ensure_ao(s, a.out_n, stream_capturing(st));   // (counts are indexed as the output is)
    const mcpt::AoUnits u = mcpt::ao_units(a.points, a.kp.spp, static_cast<uint32_t>(q.unit_samples));
    a.unit = u.unit;
    a.upp = u.upp;
    a.div_upp = mcpt::FastDiv::make(u.upp);
    a.total_units = static_cast<uint32_t>(uint64_t(a.points) * u.upp);
    a.counts = static_cast<uint32_t*>(s.ao_counts.p);
    a.spill = static_cast<uint4*>(s.ws.spill.p);
    a.spill_stride = static_cast<uint32_t>(launched_lanes(s));
    a.stats = host_block ? query_blocks(s)->host : query_blocks(s)->device;
    a.refill = q.refill;
    a.radius = q.radius;
    a.bias = q.bias;
    HIP_TRY(mcpt::launch_ao(a, q.lean != 0, s.cus, q.workgroups, st));
}

void ao_points_async(mcpt_scene& s, const mcpt_ao_params& q, int64_t n, const float* d_p, const float* d_n,
                     const uint32_t* d_stream, float* d_ao, bool host_block, hipStream_t st) {
    mcpt::AoParams a{};
    a.kp.scene = s.gpu;
    a.kp.spp = q.spp;
    a.kp.spp_offset = q.spp_offset;
    a.kp.prev_count = q.prev_count;
    a.kp.key = tea16(static_cast<uint32_t>(q.seed), static_cast<uint32_t>(q.seed >> 32));
    a.p = d_p;
    a.nrm = d_n;
    a.stream = d_stream;
    a.out = d_ao;
    a.points = a.out_n = static_cast<uint32_t>(n);
    a.pixel = 0;
    ao_async(s, q, a, host_block, st);
}

void ao_frame_async(mcpt_scene& s, const AoFrame& F, float* d_ao, bool host_block, hipStream_t st) {
    mcpt::AoParams a{};
    a.kp = make_plan(s, &F.rp).kp;        // (one shard, whole tiles, CVMCTracer mode: ao_frame_resolve)
    a.out = d_ao;
    a.points = a.kp.npix_local;
    a.out_n = static_cast<uint32_t>(F.rp.width) * static_cast<uint32_t>(F.rp.height);
    a.pixel = 1;
    ao_async(s, F.q, a, host_block, st);
}

// ---- direct-lighting queries (direct.hip) -----------------------------------------
// The checks of a direct-lighting query's own params, p resolved (NULL = the
// defaults) with its zero bias replaced
mcpt_direct_params direct_fields(const mcpt_direct_params* p) {
    mcpt_direct_params q;
    mcpt_direct_params_default(&q);
    if (p) q = *p;
    if (q.spp == 0) throw mcpt::Error{MCPT_E_INVALID, "spp must be >= 1"};
    if (uint64_t(q.spp_offset) + uint64_t(q.spp) > (uint64_t(1) << 32))
        throw mcpt::Error{MCPT_E_INVALID, "spp_offset + spp must not pass 2^32"};
    if (!std::isfinite(q.illum)) throw mcpt::Error{MCPT_E_INVALID, "illum must be finite"};
    if (!(q.bias >= 0.0f) || !std::isfinite(q.bias))
        throw mcpt::Error{MCPT_E_INVALID, "bias must be > 0 and finite (0 = 0.01)"};
    if (q.lean != 0 && q.lean != 1) throw mcpt::Error{MCPT_E_INVALID, "lean must be 0 or 1"};
    if (q.workgroups < 0) throw mcpt::Error{MCPT_E_INVALID, "workgroups must be >= 0"};
    if (q.refill < 0 || q.refill > 64) throw mcpt::Error{MCPT_E_INVALID, "refill must be 0 (default) or 1..64"};
    if (q.bias == 0.0f) q.bias = 0.01f;
    return q;
}
// samples per chunk and chunks per point of spp samples in chunks of spp_chunk (0 = spp)
struct DirectChunks {
    uint32_t chunk;
    uint64_t chunks;
};
DirectChunks direct_chunks(uint32_t spp, uint32_t spp_chunk) {
    const uint32_t chunk = spp_chunk ? (spp_chunk < spp ? spp_chunk : spp) : spp;
    return DirectChunks{chunk, (uint64_t(spp) + chunk - 1) / chunk};
}
// The checks of the point form that need no device, in the header's order
mcpt_direct_params direct_resolve(const mcpt_scene* s, const mcpt_direct_params* p, int64_t n, bool ptrs) {
    if (!s) throw mcpt::Error{MCPT_E_INVALID, "NULL scene"};
    if (n < 0) throw mcpt::Error{MCPT_E_INVALID, "n must be >= 0"};
    if (n && !ptrs) throw mcpt::Error{MCPT_E_INVALID, "NULL point, normal or result buffer"};
    const mcpt_direct_params q = direct_fields(p);
    if (n >= (int64_t(1) << 31) / 3) throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many points for one call"};
    if (uint64_t(n) * direct_chunks(q.spp, q.spp_chunk).chunks >= (uint64_t(1) << 31))
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many work units (points x chunks) for one call"};
    if (!s->on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    return q;
}
// ... and of the pixel form (frame_resolve): the frame's samples in the direct params' chunks
struct DirectFrame {
    mcpt_render_params rp;
    mcpt_direct_params q;
};
DirectFrame direct_frame_resolve(const mcpt_scene* s, const mcpt_render_params* rp, const mcpt_direct_params* dp,
                                 bool ptr) {
    DirectFrame F;
    F.rp = frame_resolve(s, rp, ptr, "direct lighting", [&] {
        F.q = direct_fields(dp);
        return FrameQuery{F.q.lean, direct_chunks(rp->spp, F.q.spp_chunk).chunks};
    });
    return F;
}

// What the direct-lighting queries need on the scene's (current) device for `units`
// (point or pixel, chunk) units of a query in `chunks` chunks: the ray queries'
// (ensure_rays), the kernels, and with more than one chunk a partial sum per unit.
// The light table came with the scene.  Nothing once they exist.
void ensure_direct(mcpt_scene& s, uint64_t units, uint64_t chunks, bool capturing) {
    if (capturing && (!s.rq_order.p || !s.rq_stats.p || !s.dl_prepared))
        throw mcpt::Error{MCPT_E_NOMEM, "the first direct-lighting query of a scene allocates: call "
                                        "mcpt_scene_reserve_direct before capturing a graph"};
    ensure_rays(s, capturing);
    if (!s.dl_prepared) {
        HIP_TRY(mcpt::prepare_direct(s.gpu));         // (the kernels' code object loaded now)
        s.dl_prepared = true;
    }
    if (chunks > 1) grow_ws(s, s.dl_partial, static_cast<size_t>(units) * 16, capturing);
}

// One query on st over a filled d.kp (d.p, d.nrm, d.stream, d.out, d.points, d.out_n, d.pixel, d.bias set)
void direct_async(mcpt_scene& s, const mcpt_direct_params& q, mcpt::DirectParams& d, bool host_block,
                  hipStream_t st) {
    const DirectChunks ch = direct_chunks(d.kp.spp, q.spp_chunk);
    // (partial sums are indexed as the output is: chunk x out_n + point)
    ensure_direct(s, uint64_t(d.out_n) * ch.chunks, ch.chunks, stream_capturing(st));
    d.chunk = ch.chunk;
    d.chunks = static_cast<uint32_t>(ch.chunks);
    d.div_chunks = mcpt::FastDiv::make(d.chunks);
    d.total_units = static_cast<uint32_t>(uint64_t(d.points) * ch.chunks);
    d.partial = static_cast<float4*>(s.dl_partial.p);
    const size_t L = s.lights.kd_ids.size();
    d.n_lights = static_cast<uint32_t>(L);
    d.lights = static_cast<const float4*>(s.d_lights.p);
    d.cdf = L ? static_cast<const float*>(s.d_lights.p) + L * (mcpt::kLightRecordBytes / 4) : nullptr;
    d.area_total = s.lights.area_total;
    d.illum = q.illum;
    d.spill = static_cast<uint4*>(s.ws.spill.p);
    d.spill_stride = static_cast<uint32_t>(launched_lanes(s));
    d.stats = host_block ? query_blocks(s)->host : query_blocks(s)->device;
    d.refill = q.refill;
    HIP_TRY(mcpt::launch_direct(d, q.lean != 0, s.cus, q.workgroups, st));
}

void direct_points_async(mcpt_scene& s, const mcpt_direct_params& q, int64_t n, const float* d_p, const float* d_n,
                         const uint32_t* d_stream, float* d_out, bool host_block, hipStream_t st) {
    mcpt::DirectParams d{};
    d.kp.scene = s.gpu;
    d.kp.spp = q.spp;
    d.kp.spp_offset = q.spp_offset;
    d.kp.prev_count = q.prev_count;
    d.kp.key = tea16(static_cast<uint32_t>(q.seed), static_cast<uint32_t>(q.seed >> 32));
    d.p = d_p;
    d.nrm = d_n;
    d.stream = d_stream;
    d.out = reinterpret_cast<float4*>(d_out);
    d.points = d.out_n = static_cast<uint32_t>(n);
    d.bias = q.bias;
    d.pixel = 0;
    direct_async(s, q, d, host_block, st);
}

void direct_frame_async(mcpt_scene& s, const DirectFrame& F, float* d_out, bool host_block, hipStream_t st) {
    mcpt::DirectParams d{};
    d.kp = make_plan(s, &F.rp).kp;        // (one shard, whole tiles, CVMCTracer mode: frame_resolve)
    d.out = reinterpret_cast<float4*>(d_out);
    d.points = d.kp.npix_local;
    d.out_n = static_cast<uint32_t>(F.rp.width) * static_cast<uint32_t>(F.rp.height);
    d.bias = 0.01f;                       // (the renders' literal)
    d.pixel = 1;
    direct_async(s, F.q, d, host_block, st);
}

}  // namespace

extern "C" {

int mcpt_direct_device(mcpt_scene* s, const mcpt_direct_params* p, int64_t n, const float* d_p, const float* d_n,
                       const uint32_t* d_stream, float* d_out, void* hip_stream) {
    return guarded([&]() -> int {
        const mcpt_direct_params q = direct_resolve(s, p, n, d_p && d_n && d_out);
        const size_t N = static_cast<size_t>(n);
        if (ranges_overlap(d_out, N * 16, d_p, N * 12) || ranges_overlap(d_out, N * 16, d_n, N * 12) ||
            ranges_overlap(d_out, N * 16, d_stream, d_stream ? N * 4 : 0))
            return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
        if (!n) return MCPT_OK;
        set_device(*s);                   // (a multi-device scene: devices[0], the primary)
        direct_points_async(*s, q, n, d_p, d_n, d_stream, d_out, false, static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

// points, normals, stream ids and the result are staged in the scene's host-render buffer
int mcpt_direct(mcpt_scene* s, const mcpt_direct_params* p, int64_t n, const float* p_xyz, const float* nrm,
                const uint32_t* stream, float* out, mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        const mcpt_direct_params q = direct_resolve(s, p, n, p_xyz && nrm && out);
        const size_t N = static_cast<size_t>(n);
        if (ranges_overlap(out, N * 12, p_xyz, N * 12) || ranges_overlap(out, N * 12, nrm, N * 12) ||
            ranges_overlap(out, N * 12, stream, stream ? N * 4 : 0))
            return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n) {
            set_device(*s);
            const auto part = carve({N * 16, N * 12, N * 12, N * 4});
            ensure_buf(s->ws.fb, part.total);
            float* d_out = part.at<float>(s->ws.fb.p, 0);
            float* d_p = part.at<float>(s->ws.fb.p, 1);
            float* d_n = part.at<float>(s->ws.fb.p, 2);
            uint32_t* d_s = part.at<uint32_t>(s->ws.fb.p, 3);
            HIP_TRY(hipMemcpy(d_p, p_xyz, N * 12, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_n, nrm, N * 12, hipMemcpyHostToDevice));
            if (stream) HIP_TRY(hipMemcpy(d_s, stream, N * 4, hipMemcpyHostToDevice));
            std::vector<float> rgba(N * 4, 0.0f);
            if (q.prev_count) {
                rgb_to_rgba(out, N, rgba.data());
                HIP_TRY(hipMemcpy(d_out, rgba.data(), N * 16, hipMemcpyHostToDevice));
            }
            ensure_rays(*s, false);       // (the counter blocks exist before the host entry's is cleared)
            unsigned long long* blk = clear_host_block(*s);
            direct_points_async(*s, q, n, d_p, d_n, stream ? d_s : nullptr, d_out, true, nullptr);
            HIP_TRY(hipStreamSynchronize(nullptr));
            HIP_TRY(hipMemcpy(rgba.data(), d_out, N * 16, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(c, blk, sizeof c, hipMemcpyDeviceToHost));
            rgba_to_rgb(rgba.data(), N, out);
        }
        if (stats) stats_from_counters(c, *stats);
        return MCPT_OK;
    });
}

int mcpt_render_direct_device(mcpt_scene* s, const mcpt_render_params* rp, const mcpt_direct_params* dp,
                              float* d_out_rgba, void* hip_stream) {
    return guarded([&]() -> int {
        const DirectFrame F = direct_frame_resolve(s, rp, dp, d_out_rgba != nullptr);
        set_device(*s);                   // (a multi-device scene: devices[0], the primary)
        direct_frame_async(*s, F, d_out_rgba, false, static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

// the result is staged in the scene's host-render buffer
int mcpt_render_direct(mcpt_scene* s, const mcpt_render_params* rp, const mcpt_direct_params* dp, float* out,
                       mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        const DirectFrame F = direct_frame_resolve(s, rp, dp, out != nullptr);
        set_device(*s);
        const size_t N = size_t(F.rp.width) * size_t(F.rp.height);
        ensure_buf(s->ws.fb, N * 16);
        float* d_out = static_cast<float*>(s->ws.fb.p);
        std::vector<float> rgba(N * 4, 0.0f);
        if (F.rp.prev_count) {
            rgb_to_rgba(out, N, rgba.data());
            HIP_TRY(hipMemcpy(d_out, rgba.data(), N * 16, hipMemcpyHostToDevice));
        }
        ensure_rays(*s, false);
        unsigned long long* blk = clear_host_block(*s);
        direct_frame_async(*s, F, d_out, true, nullptr);
        HIP_TRY(hipStreamSynchronize(nullptr));
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIP_TRY(hipMemcpy(rgba.data(), d_out, N * 16, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c, blk, sizeof c, hipMemcpyDeviceToHost));
        rgba_to_rgb(rgba.data(), N, out);
        if (stats) stats_from_counters(c, *stats);
        return MCPT_OK;
    });
}

int mcpt_scene_reserve_direct(mcpt_scene* s, const mcpt_direct_params* p, int64_t n) {
    return guarded([&]() -> int {
        if (!s || !s->on_device) return fail(MCPT_E_INVALID, "scene is not on a device");
        if (n < 0) return fail(MCPT_E_INVALID, "n must be >= 0");
        const mcpt_direct_params q = direct_fields(p);
        const uint64_t chunks = direct_chunks(q.spp, q.spp_chunk).chunks;
        if (n >= (int64_t(1) << 31) / 3) return fail(MCPT_E_UNSUPPORTED, "too many points for one call");
        if (uint64_t(n) * chunks >= (uint64_t(1) << 31))
            return fail(MCPT_E_UNSUPPORTED, "too many work units (points x chunks) for one call");
        DeviceGuard guard;
        set_device(*s);
        ensure_direct(*s, std::max<uint64_t>(uint64_t(n), 1) * chunks, chunks, false);
        return MCPT_OK;
    });
}

int mcpt_ao_device(mcpt_scene* s, const mcpt_ao_params* p, int64_t n, const float* d_p, const float* d_n,
                   const uint32_t* d_stream, float* d_ao, void* hip_stream) {
    return guarded([&]() -> int {
        const mcpt_ao_params q = ao_resolve(s, p, n, d_p && d_n && d_ao);
        const size_t N = static_cast<size_t>(n);
        if (ranges_overlap(d_ao, N * 4, d_p, N * 12) || ranges_overlap(d_ao, N * 4, d_n, N * 12) ||
            ranges_overlap(d_ao, N * 4, d_stream, d_stream ? N * 4 : 0))
            return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
        if (!n) return MCPT_OK;
        set_device(*s);                   // (a multi-device scene: devices[0], the primary)
        ao_points_async(*s, q, n, d_p, d_n, d_stream, d_ao, false, static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

// points, normals, stream ids and the result are staged in the scene's host-render buffer
int mcpt_ao(mcpt_scene* s, const mcpt_ao_params* p, int64_t n, const float* p_xyz, const float* nrm,
            const uint32_t* stream, float* ao, mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        const mcpt_ao_params q = ao_resolve(s, p, n, p_xyz && nrm && ao);
        const size_t N = static_cast<size_t>(n);
        if (ranges_overlap(ao, N * 4, p_xyz, N * 12) || ranges_overlap(ao, N * 4, nrm, N * 12) ||
            ranges_overlap(ao, N * 4, stream, stream ? N * 4 : 0))
            return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n) {
            set_device(*s);
            const auto part = carve({N * 12, N * 12, N * 4, N * 4});
            ensure_buf(s->ws.fb, part.total);
            float* d_p = part.at<float>(s->ws.fb.p, 0);
            float* d_n = part.at<float>(s->ws.fb.p, 1);
            uint32_t* d_s = part.at<uint32_t>(s->ws.fb.p, 2);
            float* d_ao = part.at<float>(s->ws.fb.p, 3);
            HIP_TRY(hipMemcpy(d_p, p_xyz, N * 12, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_n, nrm, N * 12, hipMemcpyHostToDevice));
            if (stream) HIP_TRY(hipMemcpy(d_s, stream, N * 4, hipMemcpyHostToDevice));
            if (q.prev_count) HIP_TRY(hipMemcpy(d_ao, ao, N * 4, hipMemcpyHostToDevice));
            ensure_rays(*s, false);       // (the counter blocks exist before the host entry's is cleared)
            unsigned long long* blk = clear_host_block(*s);
            ao_points_async(*s, q, n, d_p, d_n, stream ? d_s : nullptr, d_ao, true, nullptr);
            HIP_TRY(hipStreamSynchronize(nullptr));
            HIP_TRY(hipMemcpy(ao, d_ao, N * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(c, blk, sizeof c, hipMemcpyDeviceToHost));
        }
        if (stats) stats_from_counters(c, *stats);
        return MCPT_OK;
    });
}

int mcpt_render_ao_device(mcpt_scene* s, const mcpt_render_params* rp, const mcpt_ao_params* ap, float* d_ao,
                          void* hip_stream) {
    return guarded([&]() -> int {
        const AoFrame F = ao_frame_resolve(s, rp, ap, d_ao != nullptr);
        set_device(*s);                   // (a multi-device scene: devices[0], the primary)
        ao_frame_async(*s, F, d_ao, false, static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

// the result is staged in the scene's host-render buffer
int mcpt_render_ao(mcpt_scene* s, const mcpt_render_params* rp, const mcpt_ao_params* ap, float* ao,
                   mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        const AoFrame F = ao_frame_resolve(s, rp, ap, ao != nullptr);
        set_device(*s);
        const size_t bytes = size_t(F.rp.width) * size_t(F.rp.height) * 4;
        ensure_buf(s->ws.fb, bytes);
        float* d_ao = static_cast<float*>(s->ws.fb.p);
        if (F.rp.prev_count) HIP_TRY(hipMemcpy(d_ao, ao, bytes, hipMemcpyHostToDevice));
        ensure_rays(*s, false);
        unsigned long long* blk = clear_host_block(*s);
        ao_frame_async(*s, F, d_ao, true, nullptr);
        HIP_TRY(hipStreamSynchronize(nullptr));
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIP_TRY(hipMemcpy(ao, d_ao, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c, blk, sizeof c, hipMemcpyDeviceToHost));
        if (stats) stats_from_counters(c, *stats);
        return MCPT_OK;
    });
}

int mcpt_scene_reserve_ao(mcpt_scene* s, int64_t n) {
    return guarded([&]() -> int {
        if (!s || !s->on_device) return fail(MCPT_E_INVALID, "scene is not on a device");
        if (n < 0) return fail(MCPT_E_INVALID, "n must be >= 0");
        if (n >= (int64_t(1) << 31) / 3) return fail(MCPT_E_UNSUPPORTED, "too many points for one call");
        DeviceGuard guard;
        set_device(*s);
        ensure_ao(*s, static_cast<uint64_t>(n), false);
        return MCPT_OK;
    });
}

int mcpt_intersect(mcpt_scene* s, int64_t n, const float* o, const float* d, float t_max, int32_t* tri_out,
                   float* hit_out, mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        if (!s || n < 0 || (n && (!o || !d || !tri_out || !hit_out))) return fail(MCPT_E_INVALID, "NULL argument");
        if (!s->on_device) return fail(MCPT_E_INVALID, "scene was created host-only");
        if (n >= (int64_t(1) << 31) / 3) return fail(MCPT_E_UNSUPPORTED, "too many rays for one call");
        set_device(*s);
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n) {
            const size_t N = static_cast<size_t>(n);
            // one allocation: o, d, hits (3 floats each), slots, counters, then the
            // stack spill area of the old query kernel: kSpillEntries per ray, not per lane
            const auto p = carve({N * 12, N * 12, N * 12, N * 4, size_t(64), N * kSpillEntries * 16});
            TempDev buf(p.total);
            mcpt::QueryParams q{};
            q.scene = s->gpu;
            q.o = p.at<float>(buf.p, 0);
            q.d = p.at<float>(buf.p, 1);
            q.hit = p.at<float>(buf.p, 2);
            q.slot = p.at<int32_t>(buf.p, 3);
            q.stats = p.at<unsigned long long>(buf.p, 4);
            q.spill = p.at<uint4>(buf.p, 5);
            q.n = static_cast<uint32_t>(n);
            q.best_init = t_max;
            HIP_TRY(hipMemcpy(p.at<float>(buf.p, 0), o, N * 12, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(p.at<float>(buf.p, 1), d, N * 12, hipMemcpyHostToDevice));
            HIP_TRY(hipMemset(q.stats, 0, 64));
            HIP_TRY(mcpt::launch_query(q, nullptr));
            HIP_TRY(hipDeviceSynchronize());
            std::vector<int32_t> slot(N);
            HIP_TRY(hipMemcpy(slot.data(), q.slot, N * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(hit_out, q.hit, N * 12, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(c, q.stats, 64, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < N; ++i)
                tri_out[i] = slot[i] < 0 ? -1 : static_cast<int32_t>(s->tri_order[static_cast<size_t>(slot[i])]);
        }
        // (the old query kernel leaves paths and shades 0)
        if (stats) stats_from_counters(c, *stats);
        return MCPT_OK;
    });
}

int mcpt_trace_device(mcpt_scene* s, const mcpt_trace_params* p, int64_t n, const float* d_o, const float* d_d,
                      const float* d_t_max, int32_t* d_tri, float* d_hit, void* hip_stream) {
    return guarded([&]() -> int {
        const mcpt_trace_params q = trace_resolve(s, p, n, d_o && d_d && d_tri, true);
        const size_t N = static_cast<size_t>(n);
        const void* in[3] = {d_o, d_d, d_t_max};
        const size_t in_bytes[3] = {N * 12, N * 12, d_t_max ? N * 4 : 0};
        for (int i = 0; i < 3; ++i)
            if (ranges_overlap(d_tri, N * 4, in[i], in_bytes[i]) ||
                (d_hit && ranges_overlap(d_hit, N * 12, in[i], in_bytes[i])))
                return fail(MCPT_E_INVALID, "an output buffer overlaps an input of the call");
        if (d_hit && ranges_overlap(d_tri, N * 4, d_hit, N * 12))
            return fail(MCPT_E_INVALID, "the triangle and hit buffers overlap");
        if (!n) return MCPT_OK;
        set_device(*s);                   // (a multi-device scene: devices[0], the primary)
        rays_async(*s, q, n, d_o, d_d, d_t_max, d_tri, d_hit, nullptr, false, static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

int mcpt_occluded_device(mcpt_scene* s, const mcpt_trace_params* p, int64_t n, const float* d_o, const float* d_d,
                         const float* d_t_max, uint8_t* d_occluded, void* hip_stream) {
    return guarded([&]() -> int {
        const mcpt_trace_params q = trace_resolve(s, p, n, d_o && d_d && d_occluded, false);
        const size_t N = static_cast<size_t>(n);
        if (ranges_overlap(d_occluded, N, d_o, N * 12) || ranges_overlap(d_occluded, N, d_d, N * 12) ||
            ranges_overlap(d_occluded, N, d_t_max, d_t_max ? N * 4 : 0))
            return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
        if (!n) return MCPT_OK;
        set_device(*s);
        rays_async(*s, q, n, d_o, d_d, d_t_max, nullptr, nullptr, d_occluded, false,
                   static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

// rays, t_max and the flags are staged in the scene's host-render buffer
int mcpt_occluded(mcpt_scene* s, const mcpt_trace_params* p, int64_t n, const float* o, const float* d,
                  const float* t_max, uint8_t* occluded, mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        const mcpt_trace_params q = trace_resolve(s, p, n, o && d && occluded, false);
        const size_t N = static_cast<size_t>(n);
        if (ranges_overlap(occluded, N, o, N * 12) || ranges_overlap(occluded, N, d, N * 12) ||
            ranges_overlap(occluded, N, t_max, t_max ? N * 4 : 0))
            return fail(MCPT_E_INVALID, "the output buffer overlaps an input of the call");
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n) {
            set_device(*s);
            const auto part = carve({N * 12, N * 12, N * 4, N});
            ensure_buf(s->ws.fb, part.total);
            float* d_o = part.at<float>(s->ws.fb.p, 0);
            float* d_d = part.at<float>(s->ws.fb.p, 1);
            float* d_t = part.at<float>(s->ws.fb.p, 2);
            uint8_t* d_occ = part.at<uint8_t>(s->ws.fb.p, 3);
            HIP_TRY(hipMemcpy(d_o, o, N * 12, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_d, d, N * 12, hipMemcpyHostToDevice));
            if (t_max) HIP_TRY(hipMemcpy(d_t, t_max, N * 4, hipMemcpyHostToDevice));
            ensure_rays(*s, false);
            unsigned long long* blk = clear_host_block(*s);
            rays_async(*s, q, n, d_o, d_d, t_max ? d_t : nullptr, nullptr, nullptr, d_occ, true, nullptr);
            HIP_TRY(hipStreamSynchronize(nullptr));
            HIP_TRY(hipMemcpy(occluded, d_occ, N, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(c, blk, sizeof c, hipMemcpyDeviceToHost));
        }
        if (stats) stats_from_counters(c, *stats);
        return MCPT_OK;
    });
}

int mcpt_trace_stats_read(mcpt_scene* s, mcpt_render_stats* out) {
    return guarded([&]() -> int {
        if (!s || !s->on_device) return fail(MCPT_E_INVALID, "scene is not on a device");
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // ... and with them the routes the wavefront radiance queries' rays took (mcpt_scene_query_route_rays)
        unsigned long long r[mcpt::kQueryRoutes] = {};
        if (s->rq_stats.p) {              // (no query yet: zeros)
            DeviceGuard guard;
            set_device(*s);
            // the queries may run on any stream: wait for the device, then read and clear
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(c, query_blocks(*s)->device, sizeof c, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemset(query_blocks(*s)->device, 0, sizeof c));
            if (s->rad_wf_stats.p) {
                HIP_TRY(hipMemcpy(r, wf_query_block(*s)->routes, sizeof r, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemset(wf_query_block(*s)->routes, 0, sizeof r));
            }
        }
        for (int i = 0; i < mcpt::kQueryRoutes; i++) s->query_routes[i] = r[i];
        if (out) stats_from_counters(c, *out);
        return MCPT_OK;
    });
}

int mcpt_scene_reserve_rays(mcpt_scene* s) {
    return guarded([&]() -> int {
        if (!s || !s->on_device) return fail(MCPT_E_INVALID, "scene is not on a device");
        DeviceGuard guard;
        set_device(*s);
        ensure_rays(*s, false);
        return MCPT_OK;
    });
}

int mcpt_radiance_device(mcpt_scene* s, const mcpt_radiance_params* p, int64_t n, const float* d_o, const float* d_d,
                         const uint32_t* d_stream, float* d_radiance, void* hip_stream) {
    return guarded([&]() -> int {
        const Radiance R = radiance_resolve(s, p, n, d_o && d_d && d_radiance);
        return radiance_device(s, R, nullptr, n, d_o, d_d, d_stream, d_radiance, hip_stream);
    });
}

int mcpt_radiance(mcpt_scene* s, const mcpt_radiance_params* p, int64_t n, const float* o, const float* d,
                  const uint32_t* stream, float* radiance, mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        const Radiance R = radiance_resolve(s, p, n, o && d && radiance);
        return radiance_host(s, R, n, o, d, stream, radiance, stats,
                             [&](const float* d_o, const float* d_d, const uint32_t* d_s, float* d_out) {
                                 radiance_async(*s, R, n, d_o, d_d, d_s, d_out, true, nullptr);
                                 return 0;
                             });
    });
}

int mcpt_scene_reserve_radiance(mcpt_scene* s, const mcpt_radiance_params* p, int64_t n) {
    return guarded([&]() -> int {
        const Radiance R = radiance_resolve(s, p, n, true);
        DeviceGuard guard;
        set_device(*s);
        uint64_t tail = 0;
        mcpt::KernelParams k = radiance_plan(*s, R, n, &tail);
        ensure_radiance(*s, k, tail, false, false);
        return MCPT_OK;
    });
}

int mcpt_radiance_ex_device(mcpt_scene* s, const mcpt_radiance_ex_params* p, int64_t n, const float* d_o,
                            const float* d_d, const uint32_t* d_stream, float* d_radiance, void* hip_stream) {
    return guarded([&]() -> int {
        const RadianceEx E = radiance_ex_resolve(s, p, n, d_o && d_d && d_radiance);
        return radiance_device(s, E.R, E.wavefront() ? &E : nullptr, n, d_o, d_d, d_stream, d_radiance, hip_stream);
    });
}

int mcpt_radiance_ex(mcpt_scene* s, const mcpt_radiance_ex_params* p, int64_t n, const float* o, const float* d,
                     const uint32_t* stream, float* radiance, mcpt_render_stats* stats) {
    return guarded([&]() -> int {
        const RadianceEx E = radiance_ex_resolve(s, p, n, o && d && radiance);
        return radiance_host(s, E.R, n, o, d, stream, radiance, stats,
                             [&](const float* d_o, const float* d_d, const uint32_t* d_s, float* d_out) {
                                 if (E.wavefront()) return radiance_wf_async(*s, E, n, d_o, d_d, d_s, d_out, true, nullptr);
                                 radiance_async(*s, E.R, n, d_o, d_d, d_s, d_out, true, nullptr);
                                 return 0;
                             });
    });
}

// (the wavefront form reserves as mcpt_scene_reserve does for a render: the workspace is
// the renders', and from here on a buffer that grows is retired, not freed)
int mcpt_scene_reserve_radiance_ex(mcpt_scene* s, const mcpt_radiance_ex_params* p, int64_t n) {
    return guarded([&]() -> int {
        const RadianceEx E = radiance_ex_resolve(s, p, n, true);
        DeviceGuard guard;
        set_device(*s);
        if (!E.wavefront()) {
            uint64_t tail = 0;
            mcpt::KernelParams k = radiance_plan(*s, E.R, n, &tail);
            ensure_radiance(*s, k, tail, false, false);
            return MCPT_OK;
        }
        if (!n) return MCPT_OK;
        s->reserved = true;
        Prepared P;
        prepare_radiance_wf(*s, E, n, false, P);
        // (the kernels' code objects loaded now: the reduce's, the pipeline's, the ray frame's)
        HIP_TRY(mcpt::prepare_radiance(s->gpu));
        HIP_TRY(mcpt::load_wavefront(P.pl.route));
        HIP_TRY(mcpt::load_wavefront_rays());
        s->wf_reserved = std::max(s->wf_reserved, s->ws.wf.bytes);
        return MCPT_OK;
    });
}

int mcpt_scene_query_route_rays(const mcpt_scene* s, uint64_t out[4]) {
    if (!s || !out) return fail(MCPT_E_INVALID, "NULL argument");
    for (int i = 0; i < mcpt::kQueryRoutes; i++) out[i] = s->query_routes[i];
    return MCPT_OK;
}

}  // extern "C"
