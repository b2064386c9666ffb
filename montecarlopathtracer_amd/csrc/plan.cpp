// plan.cpp -- the plan of a render and the workspace it runs in: how the frame
// is cut into work units, which pipeline and batch sizes it uses (the measured
// sweeps behind each default are kept with the code), what the scene has to
// hold for it and how that is grown; mcpt_plan_query and the shard entries
// report from the same functions.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>

#include "capi_internal.hpp"

using namespace mcpt::host;

namespace {

struct Vf {
    float x, y, z;
};
// Math::Vector3f::normal()/cross() (CVMCTracer/Framework/Math.hpp:112-123)
Vf normal_of(Vf v) {
    float len = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    float d = std::fmax(len, FLT_MIN);
    return Vf{v.x / d, v.y / d, v.z / d};
}
Vf cross_of(Vf a, Vf b) { return Vf{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// wavefront streams: 2-3 for scenes in LDS, 4 for scenes in global memory (C2
// 1024 spp, streams x batch: 2 x 2^27 11.48, 2 x 2^26 11.46, 4 x 2^27 11.52,
// 4 x 2^26 10.93; C4 1024 spp: 1 x 2^28 6.14, 2 x 2^28 8.07, 3 x 2^27 8.17,
// 4 x 2^27 8.28 G rays/s, means of 2-3 runs).  mcpt_render_params::wf_streams
// (1..4) overrides; 1 = every batch on the caller's stream.
// LDS scenes: 3 streams for frames of more than 2^29 paths (C2 after the
// id-only hit records: 2 x 2^28 13.48 / 13.45, 3 x 2^27 13.65 / 13.56,
// 3 x 2^30/9 13.65 / 13.59 G rays/s), 2 up to 2^29 (one rank's C2 share at
// N = 2, 2^29 paths: 136.1 ms on 2 x 2^27, 136.7 on 2 x 2^28, 143.3 on
// 3 x 2^27 -- four batches on three streams leave one alone at the end; at
// N = 8, 2^27 paths: 35.4 ms on 2 streams, 37.6 on 3)
// Renders whose queue-order shade carries the rays it resolves (lean, direct
// lists active, wf_sort = 0: render_launch.hpp "Direct resolve") do most of
// their shading in the first bounces' kernels, and two streams of 2^28 suit
// them at every size (C2, ms per frame, one round of 10 frames: 2 x 2^28 145.5,
// 3 x 2^27 157.9, 4 x 2^27 153.3, 3 x 2^26 168.3, 4 x 2^26 160.0, 1 x 2^28
// 168.6; the commit before the carry 152.6 / 149.7 / 149.2 / 159.4 / 149.9;
// PERFLOG row 184)
int wavefront_streams(const mcpt::WfRoute& r, uint64_t work, const mcpt_render_params* p) {
    const int n = p->wf_streams > 0 ? p->wf_streams
                                    : (!r.in_lds ? 4 : (work > (uint64_t(1) << 29) && !r.carry ? 3 : 2));
    return clamp_i(n, 1, mcpt::kMaxWfStreams);
}

// the primary lists' tile records: one per owned 8x8 tile (wf_layout makes room, the route asks)
bool tile_records(const mcpt::KernelParams& kp) { return kp.tile == 8 && (kp.npix_local >> 6) != 0; }

// The route of the wavefront render pl plans (wf_route.hpp), from what the
// scene holds and what make_plan read; listed: a frame over a pixel list
mcpt::WfRoute plan_route(const mcpt_scene& s, const Plan& pl, uint32_t group_shift, bool listed) {
    const mcpt::KernelParams& k = pl.kp;
    mcpt::WfFacts f = scene_facts(s);
    // a culled ray stands for color * (0 * illum) = 0: illum must be finite,
    // and so must the throughput, a product of at most max_depth Kd / Ks
    // components (each rounding grows it by 2^-24 at most: 2^127 leaves room)
    const bool zero = std::isfinite(k.illum) && std::log2(std::max(1.0, double(s.tables.cull_gain))) * k.max_depth < 127.0;
    if (!zero) f.n_cull_boxes = 0;
    f.lean = k.lean != 0;
    f.sort = pl.wf_sort != 0;
    f.qe = k.mode == MCPT_MODE_QUINENGINE;
    f.listed = listed;
    f.default_batch = !pl.wf_batch_explicit;
    f.tile_records = tile_records(k);
    f.tile = k.tile;
    f.max_depth = k.max_depth;
    f.group_shift = group_shift;
    return mcpt::wf_route(f);
}

// Device memory of one stream's wavefront workspace for batches of `cap`
// paths (prepare_wavefront carves it): two ray queues, radiance, per-bounce
// counters.  A queue is three float4 streams (origin + path id, direction +
// depth, throughput + RNG state) and the hit stream of 4-B triangle ids
// (wavefront.hip kQHIT): 3 x 16 + 4 B per slot and queue, 120 B per path with
// the radiance (the material sort too: it sorts in LDS).  Segments hold
// whole path groups (2^group_shift paths: 64 for LDS scenes, up to 2^14 for
// global-memory ones): up to one group of slots per segment beyond the paths.
// Each stream's part also has room for the primary lists' tile records
// (render_launch.hpp "Primary lists"; one record per owned 8x8 tile, only
// the first stream's is used), so the records come out of the same plan and
// reservation as the queues.
struct WfLayout {
    size_t cap_slots, f4, queue, tiles, need;
};
WfLayout wf_layout(const Plan& pl, uint64_t cap) {
    const mcpt::KernelParams& kp = pl.kp;
    const size_t nseg = pl.route.nseg;
    const size_t bounces = (size_t(pl.route.queries) + 1) * nseg;
    auto al256 = [](size_t x) { return (x + 255) & ~size_t(255); };
    WfLayout l;
    l.cap_slots = size_t(cap) + (nseg << pl.route.group_shift);
    l.f4 = l.cap_slots * 16;
    l.queue = al256(3 * l.f4 + 4 * l.cap_slots);
    l.tiles = tile_records(kp) ? al256(size_t(kp.npix_local >> 6) * mcpt::kListRecWords * 4) : 0;
    l.need = al256(2 * l.queue + l.f4 + l.tiles + bounces * sizeof(mcpt::WfCounters) + 256);
    return l;
}

// wavefront workspace: 2 ray queues (o, d float4), hits, 4 class lists,
// path state and radiance, per-bounce counters -- carved from one buffer, once
// per stream (`sets`: batches rotate over the wavefront's streams, each with its own)
void prepare_wavefront(mcpt_scene& s, const Plan& pl, int sets, mcpt::WfParams* out) {
    const WfLayout l = wf_layout(pl, pl.wf_capacity);
    const mcpt::WfRoute& r = pl.route;
    grow_ws(s, s.ws.wf, l.need * size_t(sets), pl.capturing);
    // a default-batch render that grew the queues past the reservation: the
    // grown queues are the reservation now (a later captured render of the same
    // params allocates nothing and must not be refused)
    if (s.reserved) s.wf_reserved = std::max(s.wf_reserved, s.ws.wf.bytes);
    for (int h = 0; h < sets; ++h) {
        char* b = static_cast<char*>(s.ws.wf.p) + size_t(h) * l.need;
        mcpt::WfParams& w = out[h];
        std::memset(&w, 0, sizeof w);
        w.q[0] = reinterpret_cast<float4*>(b); b += l.queue;
        w.q[1] = reinterpret_cast<float4*>(b); b += l.queue;
        w.radiance = reinterpret_cast<float4*>(b); b += l.f4;
        w.tile_cand = l.tiles ? reinterpret_cast<uint32_t*>(b) : nullptr; b += l.tiles;
        w.tile_classes = tile_classes(s);
        w.cnt = reinterpret_cast<mcpt::WfCounters*>(b);
        w.capacity = pl.wf_capacity;                   // paths per batch (pid range)
        w.slot_stride = static_cast<uint32_t>(l.cap_slots);
        w.refill_thresh = clamp_i(pl.wf_refill, 1, 64);
        w.sort = pl.wf_sort;
        // what the route decided, once for every batch
        w.nseg = r.nseg;
        w.group_shift = r.group_shift;
        w.xcd_deal = r.xcd_deal;
        w.shade_cull = r.shade_cull ? 1u : 0u;
        w.n_cull_boxes = r.n_cull_boxes;
        const RouteTables& t = s.tables;
        std::memcpy(w.cull_box, t.cull_box, sizeof w.cull_box);
        w.n_miss_boxes = r.n_miss_boxes;
        std::memcpy(w.miss_box, t.miss_box, sizeof w.miss_box);
        w.direct_counts = r.direct_counts;
        std::memcpy(w.direct_list, t.direct_list, sizeof w.direct_list);
    }
}

// the wavefront's side streams and their fork / join events (created once per
// scene, outside any stream capture: mcpt_scene_reserve's prepare_render makes them too)
void ensure_wf_streams(mcpt_scene& s, int n) {
    if (n > 1 && !s.wf_fork) HIP_TRY(hipEventCreateWithFlags(&s.wf_fork, hipEventDisableTiming));
    for (int i = 1; i < n; i++) {
        if (!s.wf_stream[i]) HIP_TRY(hipStreamCreateWithFlags(&s.wf_stream[i], hipStreamNonBlocking));
        if (!s.wf_join[i]) HIP_TRY(hipEventCreateWithFlags(&s.wf_join[i], hipEventDisableTiming));
    }
}

}  // namespace

namespace mcpt::host {

void ensure_buf(DevBuf& b, size_t need) {
    if (b.bytes >= need && b.p) return;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    HIP_TRY(hipMalloc(&b.p, need ? need : 16));
    b.bytes = need;
}

// A workspace buffer of scene s grown to `need` bytes.  Once the scene has been
// reserved (mcpt_scene_reserve), the old buffer is retired instead of freed --
// a HIP graph captured against it keeps valid memory (its replays use the old
// buffers, later renders the new ones) -- and on a capturing stream nothing is
// allocated at all: a captured render that needs more than the scene holds
// fails with MCPT_E_NOMEM before any launch (reserve for its params first).
void grow_ws(mcpt_scene& s, DevBuf& b, size_t need, bool capturing) {
    if (b.bytes >= need && b.p) return;
    if (capturing)
        throw mcpt::Error{MCPT_E_NOMEM, "render needs more workspace than the scene holds while its stream is "
                                        "capturing a graph: call mcpt_scene_reserve with these params first"};
    if (b.p && s.reserved) {
        s.retired.push_back(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    ensure_buf(b, need);
}

void set_device(const mcpt_scene& s) {
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != s.device) HIP_TRY(hipSetDevice(s.device));
}

bool stream_capturing(hipStream_t st) {
    if (!st) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cs));
    return cs != hipStreamCaptureStatusNone;
}

uint32_t tea16(uint32_t v0, uint32_t v1) {   // MCRT/QuinEngine/Shader/rtx.hlsl:61-72
    uint32_t sum = 0;
    for (int n = 0; n < 16; n++) {
        sum += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + sum) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}

// lanes ready before a shading round: scenes in LDS 32 (sweep 16..48);
// scenes in global memory 40 (C4: 24 5.15, 32 5.38, 40 5.50, 48 5.39 G rays/s)
int ready_thresh_for(const mcpt_scene& s, int32_t asked) { return asked > 0 ? asked : (mcpt::scene_in_lds(s.gpu) ? 32 : 40); }

size_t launched_lanes(const mcpt_scene& s) { return static_cast<size_t>(mcpt::total_lanes_for(s.gpu, s.cus)); }

mcpt::WfFacts scene_facts(const mcpt_scene& s) {   // (the render's facts: false / 0)
    const RouteTables& t = s.tables;
    mcpt::WfFacts f{&s.gpu, t.n_miss_boxes, t.direct_counts, t.n_cull_boxes, s.cus};
    f.clip_spheres = t.clip_spheres;
    f.clip_sphere = t.clip_sphere;
    return f;
}

// The traversal's stack spill area: kSpillEntries 16-B entries per launched
// lane, which the kernels index by lane -- once per set of concurrently running
// extends (the wavefront's streams: one spill area each).  Every launch that
// spills sizes it here, so no site can fall behind the lanes a kernel launches.
size_t spill_bytes(const mcpt_scene& s, int sets) { return size_t(sets) * kSpillEntries * launched_lanes(s) * 16; }
void grow_spill(mcpt_scene& s, int sets, bool capturing) { grow_ws(s, s.ws.spill, spill_bytes(s, sets), capturing); }

// The camera of p as the kernels take it: make_plan's, and the temporal
// accumulation's for both of its frames (capi.cpp)
mcpt::CameraConsts camera_consts(const mcpt_render_params& p) {
    mcpt::CameraConsts c{};
    const float a = p.fov_deg * 3.14159265359f / 360;   // CUTracer.cu:189,202
    c.tan_half_fov = static_cast<float>(std::tan(static_cast<double>(a)));
    // camera basis (CUTracer.cu:349-359)
    Vf d = normal_of(Vf{p.dir[0], p.dir[1], p.dir[2]});
    Vf r = normal_of(cross_of(d, Vf{p.up[0], p.up[1], p.up[2]}));
    Vf u = normal_of(cross_of(r, d));
    for (int i = 0; i < 3; ++i) c.eye[i] = p.eye[i];
    c.fwd[0] = d.x; c.fwd[1] = d.y; c.fwd[2] = d.z;
    c.up[0] = u.x; c.up[1] = u.y; c.up[2] = u.z;
    c.right[0] = r.x; c.right[1] = r.y; c.right[2] = r.z;
    if (p.mode == MCPT_MODE_QUINENGINE) {
        // camera GraphicsRTX.cpp:173-184 (PerspectiveFovRH: fov_deg is the vertical FOV)
        const float ys = static_cast<float>(1.0 / std::tan(static_cast<double>(a)));
        c.proj22 = ys;
        c.proj11 = ys / (static_cast<float>(p.width) / static_cast<float>(p.height));
    }
    return c;
}

Plan make_plan(const mcpt_scene& s, const mcpt_render_params* p) {
    if (!p) throw mcpt::Error{MCPT_E_INVALID, "params is NULL"};
    if (p->width <= 0 || p->height <= 0) throw mcpt::Error{MCPT_E_INVALID, "width/height must be positive"};
    if (p->spp == 0) throw mcpt::Error{MCPT_E_INVALID, "spp must be > 0"};
    if (p->max_depth < 0 || p->max_depth > mcpt::kMaxDepthParam) throw mcpt::Error{MCPT_E_INVALID, "max_depth out of range"};
    if (p->wf_streams < 0 || p->wf_streams > mcpt::kMaxWfStreams)
        throw mcpt::Error{MCPT_E_INVALID, "wf_streams must be 0 (automatic) or 1..4"};
    if (p->wf_refill < 0 || p->wf_refill > 64 || p->ready_thresh < 0 || p->ready_thresh > 64)
        throw mcpt::Error{MCPT_E_INVALID, "wf_refill / ready_thresh must be 0 (automatic) or 1..64"};
    if (p->wf_group_shift != 0 && (p->wf_group_shift < 6 || p->wf_group_shift > 14))
        throw mcpt::Error{MCPT_E_INVALID, "wf_group_shift must be 0 (automatic) or 6..14"};
    if (p->tail_units < 0) throw mcpt::Error{MCPT_E_INVALID, "tail_units must be >= 0"};
    // (every render path, one device or several, rejects an unknown gather)
    if (p->gather != MCPT_GATHER_PEER && p->gather != MCPT_GATHER_RCCL)
        throw mcpt::Error{MCPT_E_INVALID, "unknown gather"};
    const int T = p->tile > 0 ? p->tile : 8;
    if (T > 256) throw mcpt::Error{MCPT_E_INVALID, "tile too large"};
    const int sc = p->shard_count > 1 ? p->shard_count : 1;
    const int si = sc > 1 ? p->shard_index : 0;
    if (si < 0 || si >= sc) throw mcpt::Error{MCPT_E_INVALID, "shard_index out of range"};
    const uint64_t tiles_x = (uint64_t(p->width) + T - 1) / T, tiles_y = (uint64_t(p->height) + T - 1) / T;
    const uint64_t ntiles = tiles_x * tiles_y;
    const uint64_t owned = uint64_t(si) < ntiles ? (ntiles - uint64_t(si) + uint64_t(sc) - 1) / uint64_t(sc) : 0;
    const uint64_t npix = owned * uint64_t(T) * uint64_t(T);
    const uint32_t chunk = p->spp_chunk ? (p->spp_chunk < p->spp ? p->spp_chunk : p->spp) : p->spp;
    const uint64_t nchunks = (uint64_t(p->spp) + chunk - 1) / chunk;
    if (npix * nchunks >= 0xFFFFFFFFull) throw mcpt::Error{MCPT_E_UNSUPPORTED, "too many work units for one call"};

    Plan pl;
    mcpt::KernelParams& k = pl.kp;
    std::memset(&k, 0, sizeof k);
    k.scene = s.gpu;
    k.width = p->width; k.height = p->height;
    k.tile = T; k.tiles_x = static_cast<int32_t>(tiles_x);
    k.shard_count = sc; k.shard_index = si;
    k.packed = (p->packed || sc > 1) ? 1 : 0;
    k.npix_local = static_cast<uint32_t>(npix);
    k.spp = p->spp; k.spp_offset = p->spp_offset; k.chunk = chunk;
    k.nchunks = static_cast<uint32_t>(nchunks);
    k.total_units = static_cast<uint32_t>(npix * nchunks);
    k.div_npix = mcpt::FastDiv::make(std::max<uint32_t>(k.npix_local, 1));
    k.div_tt = mcpt::FastDiv::make(static_cast<uint32_t>(T * T));
    k.div_tiles_x = mcpt::FastDiv::make(static_cast<uint32_t>(tiles_x));
    k.div_tile = mcpt::FastDiv::make(static_cast<uint32_t>(T));
    k.div_chunk = mcpt::FastDiv::make(chunk);
    k.tail_units = k.total_units;         // no tail split unless prepare_workspace sets one
    k.total_items = k.total_units;
    k.max_depth = p->max_depth;
    k.lean = p->lean ? 1 : 0;
    k.illum = p->illum;
    const mcpt::CameraConsts cam = camera_consts(*p);
    k.tan_half_fov = cam.tan_half_fov;
    k.h_over_w = 1.0 * static_cast<double>(static_cast<uint32_t>(p->height)) / static_cast<double>(static_cast<uint32_t>(p->width));
    k.inv_w_pow2 = (p->width > 0 && (p->width & (p->width - 1)) == 0) ? 1.0 / static_cast<double>(p->width) : 0.0;
    k.fresnel_kd = p->fresnel_kd ? 1 : 0;
    k.prev_count = p->prev_count;
    for (int i = 0; i < 3; ++i) {
        k.eye[i] = cam.eye[i];
        k.fwd[i] = cam.fwd[i];
        k.up[i] = cam.up[i];
        k.right[i] = cam.right[i];
    }
    if (p->mode != MCPT_MODE_CVMCTRACER && p->mode != MCPT_MODE_QUINENGINE)
        throw mcpt::Error{MCPT_E_INVALID, "unknown mode"};
    k.mode = p->mode;
    k.best_init = FLT_MAX;
    if (p->mode == MCPT_MODE_QUINENGINE) {
        // rtx.hlsl:380 seeds TEA-16 with the 32-bit frame seed itself; t_best 10000 (:88);
        // the camera's projection: camera_consts
        k.key = static_cast<uint32_t>(p->seed);
        k.best_init = 10000.0f;
        k.proj22 = cam.proj22;
        k.proj11 = cam.proj11;
    } else {
        k.key = tea16(static_cast<uint32_t>(p->seed), static_cast<uint32_t>(p->seed >> 32));
    }
    k.ready_thresh = ready_thresh_for(s, p->ready_thresh);
    pl.out_pixels = k.packed ? size_t(npix) : size_t(p->width) * size_t(p->height);
    if (p->pipeline != MCPT_PIPELINE_MEGAKERNEL && p->pipeline != MCPT_PIPELINE_WAVEFRONT)
        throw mcpt::Error{MCPT_E_INVALID, "unknown pipeline"};
    pl.pipeline = p->pipeline;
    // tail split: 4 units per lane (a whole frame +0.3% over 6; rank 0 of 8
    // shards at 97.0% of ideal, 6: 96.5%, 8: 95.7%, 10: 94.8%)
    pl.tail_per_lane = p->tail_units_per_lane == 0 ? kTailPerLane : p->tail_units_per_lane;
    pl.tail_exact = p->tail_units;
    plan_wavefront(s, pl, p, false);
    return pl;
}

// The wavefront fields of the plan of a frame whose kp make_plan (or a radiance query,
// queries.cpp) has filled: knobs, route, streams and the batch before it is fitted to
// memory.  listed: a frame with an explicit queue 0 (WfFacts::listed)
void plan_wavefront(const mcpt_scene& s, Plan& pl, const mcpt_render_params* p, bool listed) {
    const uint64_t npix = pl.kp.npix_local;
    const uint32_t chunk = pl.kp.chunk;
    pl.wf_sort = p->wf_sort ? 1 : 0;
    // idle lanes before an extend wave refills: 16 for scenes in LDS (C2 sweep
    // 8 / 16 / 24: 10.08 / 10.28 / 10.19 G rays/s), 8 for scenes in global
    // memory (C4 256 spp, 2..40: 6.18 / 6.20 (4-12) / 6.14 (16) / 5.79 (32) / 5.53)
    pl.wf_refill = p->wf_refill > 0 ? p->wf_refill : (mcpt::scene_in_lds(s.gpu) ? 16 : 8);
    // global-memory scenes keep whole image regions together per segment.
    // Round 4 (XCD-aware dealing, 7-entry stacks; C4 1024 spp, G rays/s):
    // 2^8 9.36, 2^9 8.39, 2^10 7.92 / 7.86, 2^11 9.70 / 9.73, 2^12 9.96 / 9.96 /
    // 9.98, 2^13 9.74, 2^14 9.83 / 9.87 / 9.85 (round 1, 256 spp: 2^14 best)
    const uint32_t group_shift = static_cast<uint32_t>(p->wf_group_shift > 0 ? p->wf_group_shift : 12);
    pl.wf_mem_limit = p->wf_mem_limit;
    const uint64_t work = std::max<uint64_t>(npix, 1) * std::max<uint64_t>(p->spp, chunk);
    pl.work = npix * p->spp;
    pl.wf_batch_explicit = p->wf_batch != 0;
    pl.route = plan_route(s, pl, group_shift, listed);
    const int nstr = wavefront_streams(pl.route, work, p);
    pl.wf_streams = nstr;
    pl.wf_capacity = wf_batch_capacity(s, p, work, chunk, nstr);
}

// Paths per wavefront batch of a frame of `work` paths (pixels x samples) on nstr
// streams, before it is fitted to memory: p->wf_batch as asked, else the default.
// Default batch: big (120 B of queues per path and stream; fewer launches,
// shorter relative tails).  One stream: C2 2^24 5.59, 2^25 6.43, 2^26 7.07,
// 2^27 7.31, 2^28 7.24; C4 (256 spp) 2^24 2.90, 2^26 3.45, 2^28 4.31 G
// rays/s.  Global-memory scenes on 4 streams: 2^27 each (see wavefront_streams);
// LDS scenes on 2 streams: 2^28 each (C2 2 x 2^27 12.90, 2 x 2^28 13.03,
// 3 x 2^27 13.06, 4 x 2^27 12.55 G rays/s, two rounds each; 86 GB of queues)
uint32_t wf_batch_capacity(const mcpt_scene& s, const mcpt_render_params* p, uint64_t work, uint32_t chunk, int nstr) {
    const bool big = nstr == 1 || (mcpt::scene_in_lds(s.gpu) && nstr == 2);
    uint64_t cap = p->wf_batch ? p->wf_batch : (big ? (1u << 28) : (1u << 27));
    // a default batch gives every stream a batch of its own (one rank's C2
    // share at 8 GPUs, 2^27 paths: one 2^27 batch 9.26, two 2^26 12.61, four
    // 2^25 12.13 G rays/s; the megakernel 11.22)
    if (!p->wf_batch && nstr > 1) cap = std::min<uint64_t>(cap, (work + nstr - 1) / nstr);
    cap = std::max<uint64_t>(cap, chunk);                        // at least one pixel per batch
    cap = std::min<uint64_t>(cap, work);
    cap = std::min<uint64_t>(cap, uint64_t(1) << 28);               // u32 slot arithmetic; 120 B per path
    return static_cast<uint32_t>(cap);
}

// A wavefront render of a frame of n listed pixels (adaptive sampling's listed
// passes), planned inside the workspace of the pass over every pixel: pl is
// make_plan of the pass's params, pass0 the fitted plan of pass 0.  The stream
// count is pass 0's; the batch is the one a frame of n pixels would get
// (an explicit wf_batch as asked), never above the capacity pass 0 was fitted
// to, so the queues, partial sums and spill areas pass 0 holds suffice and
// nothing is allocated.
void prepare_wavefront_list(mcpt_scene& s, Plan& pl, const Plan& pass0, uint32_t n, const mcpt_render_params* p,
                            mcpt::WfParams* out) {
    mcpt::KernelParams& k = pl.kp;
    k.npix_local = n;
    k.total_units = n * k.nchunks;
    k.div_npix = mcpt::FastDiv::make(n);
    pl.work = uint64_t(n) * k.spp;
    pl.wf_streams = pass0.wf_streams;
    pl.route = plan_route(s, pl, pl.route.group_shift, true);
    pl.wf_capacity = std::min(wf_batch_capacity(s, p, pl.work, k.chunk, pl.wf_streams), pass0.wf_capacity);
    prepare_workspace(s, pl, false, pl.sets());
    prepare_wavefront(s, pl, pl.sets(), out);
    ensure_wf_streams(s, pl.sets());
}

// A ray frame (a wavefront radiance query, render_launch.hpp "Ray frames") of the n =
// k.npix_local rays of k, which queries.cpp filled as for the megakernel query; p carries
// the query's wavefront fields and its spp.  Planned as a frame of n pixels x spp with an
// explicit queue 0, fitted to memory as a render is, in the scene's wavefront workspace
// -- the renders' partial sums, spill areas, queues, streams and events; the render's
// counter block is allocated with them and not written (the caller points kp.stats at the
// query's own).  What a query and mcpt_scene_reserve_radiance_ex both run.
void prepare_wavefront_rays(mcpt_scene& s, const mcpt::KernelParams& k, const mcpt_render_params* p, bool capturing,
                            Prepared& out) {
    Plan& pl = out.pl;
    pl.kp = k;
    pl.out_pixels = k.npix_local;
    pl.capturing = capturing;
    pl.pipeline = MCPT_PIPELINE_WAVEFRONT;
    pl.tail_per_lane = -1;
    pl.tail_exact = 0;
    plan_wavefront(s, pl, p, true);
    fit_wavefront(s, pl);
    prepare_workspace(s, pl, false, pl.sets());
    prepare_wavefront(s, pl, pl.sets(), out.wf);
    ensure_wf_streams(s, pl.sets());
}

// Fit the wavefront's queues into device memory: the budget is
// wf_mem_limit, or 90% of what the device has free plus what this scene's
// workspace already holds.  A default batch is halved until every stream's
// queues fit (never below one pixel's chunk); an explicit batch that does not
// fit is an error, not a failed hipMalloc half-way through a render.  A scene
// reserved with mcpt_scene_reserve fits a default batch into its reservation
// (nothing is re-allocated inside a stream capture); if even the smallest
// batch does not fit there (a reservation made for a smaller render), the
// render grows the workspace from free memory like an unreserved scene --
// except on a capturing stream, where that would allocate, so it fails.
void fit_wavefront(const mcpt_scene& s, Plan& pl) {
    if (pl.pipeline != MCPT_PIPELINE_WAVEFRONT) return;
    uint64_t budget = pl.wf_mem_limit;
    bool reserved = false;
    if (!budget) {
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        // what prepare_workspace will still allocate beside the queues (partial
        // sums, stack spill areas) comes out of the same free memory
        const mcpt::KernelParams& k = pl.kp;
        const size_t partial = size_t(k.nchunks) * k.npix_local * 16, spill = spill_bytes(s, pl.wf_streams);
        const double others = double(partial > s.ws.partial.bytes ? partial - s.ws.partial.bytes : 0) +
                              double(spill > s.ws.spill.bytes ? spill - s.ws.spill.bytes : 0);
        const double avail = (static_cast<double>(fr) + static_cast<double>(s.ws.wf.bytes)) * 0.9 - others;
        budget = avail > 0 ? static_cast<uint64_t>(avail) : 0;
        reserved = s.wf_reserved && !pl.wf_batch_explicit;
    }
    auto need = [&](uint64_t cap) { return uint64_t(wf_layout(pl, cap).need) * uint64_t(pl.wf_streams); };
    auto fit = [&](uint64_t b) {
        uint64_t cap = pl.wf_capacity;
        if (!pl.wf_batch_explicit)
            while (need(cap) > b && cap / 2 >= pl.kp.chunk && cap > (uint64_t(1) << 16)) cap /= 2;
        return cap;
    };
    uint64_t cap = fit(reserved ? std::min<uint64_t>(budget, s.wf_reserved) : budget);
    if (reserved && need(cap) > s.wf_reserved) {
        if (pl.capturing) budget = std::min<uint64_t>(budget, s.wf_reserved);
        else cap = fit(budget);
    }
    if (need(cap) > budget) {
        char msg[256];
        std::snprintf(msg, sizeof msg,
                      "wavefront queues for batches of %llu paths need %.2f GB on %d stream(s); budget %.2f GB "
                      "(wf_mem_limit, the scene's reservation or 90%% of free device memory): lower wf_batch / wf_streams",
                      static_cast<unsigned long long>(cap), need(cap) / 1e9, pl.wf_streams, budget / 1e9);
        throw mcpt::Error{MCPT_E_NOMEM, msg};
    }
    pl.wf_capacity = static_cast<uint32_t>(cap);
}

// tail_split: the megakernel hands the last Plan::tail_per_lane (default 4)
// units per lane of the work-unit order out one sample at a time
// (KernelParams::tail_units).  Without it a lane's last whole unit (32 samples,
// ~3.5 ms) set the kernel's end: at 1024 spp, rank 0 of 8 ran 64.4 ms against
// 55.5 ideal (86%); split 2 / 4 / 6 / 8 / 12 per lane: 92 / 96 / 98 / 97 / 96%,
// 1-GPU frame unchanged (442 -> 440 ms at 6).
// The tail of a launch of `lanes` lanes over total_units units of `chunk`
// samples: `exact` units if > 0, else per_lane units per lane (<= 0: none).
uint64_t tail_split(uint64_t lanes, int64_t per_lane, int64_t exact, uint32_t total_units, uint32_t chunk) {
    if (chunk <= 1) return 0;
    uint64_t tail = exact > 0 ? static_cast<uint64_t>(exact) : (per_lane > 0 ? static_cast<uint64_t>(per_lane) * lanes : 0);
    tail = std::min<uint64_t>(tail, total_units);
    // item indices and tail slots stay below 2^31
    while (tail && uint64_t(total_units - tail) + tail * chunk >= (uint64_t(1) << 31)) tail >>= 1;
    return tail;
}
uint64_t tail_units_for(const mcpt_scene& s, const Plan& pl) {
    return tail_split(launched_lanes(s), pl.tail_per_lane, pl.tail_exact, pl.kp.total_units, pl.kp.chunk);
}

void prepare_workspace(mcpt_scene& s, Plan& pl, bool tail_split, int spill_sets) {
    mcpt::KernelParams& k = pl.kp;
    grow_ws(s, s.ws.partial, size_t(k.nchunks) * k.npix_local * 16, pl.capturing);
    if (!s.ws.small.p) {
        HIP_TRY(hipMalloc(&s.ws.small.p, sizeof(mcpt::RenderBlock)));
        HIP_TRY(hipMemset(s.ws.small.p, 0, sizeof(mcpt::RenderBlock)));
        // (the fill may still be in flight on the null stream, which a replica's
        // non-blocking stream does not wait for: its kernel's counters must land after it)
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    // (the wavefront's streams run extends concurrently: one spill area each)
    grow_spill(s, spill_sets, pl.capturing);
    k.partial = static_cast<float4*>(s.ws.partial.p);
    k.counter = render_block(s)->counter;
    k.stats = render_block(s)->stats;
    k.spill = static_cast<uint4*>(s.ws.spill.p);
    k.tail_units = k.total_units;
    k.total_items = k.total_units;
    k.tail_buf = nullptr;
    if (tail_split) {
        const uint64_t tail = tail_units_for(s, pl);
        if (tail) {
            grow_ws(s, s.ws.tail, size_t(tail) * k.chunk * 16, pl.capturing);
            k.tail_units = k.total_units - static_cast<uint32_t>(tail);
            k.total_items = k.tail_units + static_cast<uint32_t>(tail * k.chunk);
            k.tail_buf = static_cast<float4*>(s.ws.tail.p);
        }
    }
}

void stats_from_counters(const unsigned long long c[mcpt::kStatCounters], mcpt_render_stats& st) {
    std::memset(&st, 0, sizeof st);
    st.devices = 1;
    st.rays = c[mcpt::kStatRays]; st.inner_visits = c[mcpt::kStatInnerVisits]; st.leaf_visits = c[mcpt::kStatLeafVisits];
    st.leaf_refs = c[mcpt::kStatLeafRefs]; st.tri_tests = c[mcpt::kStatTriTests]; st.stack_spills = c[mcpt::kStatStackSpills];
    st.paths = c[mcpt::kStatPaths]; st.shades = c[mcpt::kStatShades];   // (the hit queries leave them 0)
}

// What a render of p allocates and creates on the scene's (current) device,
// decided once for the render itself and for mcpt_scene_reserve (a captured
// graph depends on the two agreeing): the plan, fitted to memory, its workspace
// and -- the wavefront -- its queues, streams and events.  unit_counters: the
// render counts per work unit; the tail split hands units out by sample, so it
// runs without one.
void prepare_render(mcpt_scene& s, const mcpt_render_params* p, bool capturing, bool unit_counters, Prepared& out) {
    Plan& pl = out.pl;
    pl = make_plan(s, p);
    pl.capturing = capturing;
    fit_wavefront(s, pl);
    prepare_workspace(s, pl, pl.pipeline == MCPT_PIPELINE_MEGAKERNEL && !unit_counters, pl.sets());
    if (pl.pipeline != MCPT_PIPELINE_WAVEFRONT) return;
    if (unit_counters) throw mcpt::Error{MCPT_E_UNSUPPORTED, "unit counters need the megakernel pipeline"};
    prepare_wavefront(s, pl, pl.sets(), out.wf);
    ensure_wf_streams(s, pl.sets());
}

bool multi_device(const mcpt_scene& s, const mcpt_render_params* p, const uint32_t* d_unit_counters) {
    // (an RCCL gather also runs for a one-device list: a one-rank communicator)
    return (!s.replicas.empty() || (p && p->gather == MCPT_GATHER_RCCL)) && p && p->shard_count <= 1 && !p->packed &&
           !d_unit_counters;
}

// shard r of an n-way multi-device render of p: its interleaved tiles, packed
mcpt_render_params shard_params(const mcpt_render_params& p, int n, int r) {
    mcpt_render_params pr = p;
    pr.shard_count = n;
    pr.shard_index = r;
    pr.packed = 1;
    return pr;
}

}  // namespace mcpt::host

extern "C" {

int64_t mcpt_shard_pixel_count(const mcpt_render_params* p) {
    if (!p || p->width <= 0 || p->height <= 0) return fail(MCPT_E_INVALID, "bad params");
    const int64_t T = p->tile > 0 ? p->tile : 8;
    const int64_t sc = p->shard_count > 1 ? p->shard_count : 1, si = sc > 1 ? p->shard_index : 0;
    if (si < 0 || si >= sc) return fail(MCPT_E_INVALID, "shard_index out of range");
    const int64_t ntiles = ((p->width + T - 1) / T) * ((p->height + T - 1) / T);
    const int64_t owned = si < ntiles ? (ntiles - si + sc - 1) / sc : 0;
    return owned * T * T;
}

int mcpt_shard_pixels(const mcpt_render_params* p, int32_t* xy) {
    const int64_t n = mcpt_shard_pixel_count(p);
    if (n < 0) return static_cast<int>(n);
    if (!xy) return fail(MCPT_E_INVALID, "xy is NULL");
    const int64_t T = p->tile > 0 ? p->tile : 8;
    const int64_t sc = p->shard_count > 1 ? p->shard_count : 1, si = sc > 1 ? p->shard_index : 0;
    const int64_t tiles_x = (p->width + T - 1) / T;
    for (int64_t v = 0; v < n; ++v) {
        const int64_t k = v / (T * T), w = v % (T * T);
        const int64_t t = si + k * sc;
        const int64_t x = (t % tiles_x) * T + w % T, y = (t / tiles_x) * T + w / T;
        const bool in = x < p->width && y < p->height;
        xy[2 * v] = in ? static_cast<int32_t>(x) : -1;
        xy[2 * v + 1] = in ? static_cast<int32_t>(y) : -1;
    }
    return MCPT_OK;
}

int mcpt_plan_query(mcpt_scene* s, const mcpt_render_params* p, mcpt_plan_info* out) {
    return guarded([&]() -> int {
        if (!s || !s->on_device || !p || !out) return fail(MCPT_E_INVALID, "NULL argument or host-only scene");
        DeviceGuard guard;
        // a multi-device render: the plan of devices[0]'s shard (the largest)
        const bool multi = multi_device(*s, p, nullptr);
        const int n = 1 + static_cast<int>(s->replicas.size());
        const mcpt_render_params q = multi ? shard_params(*p, n, 0) : *p;
        set_device(*s);
        Plan pl = make_plan(*s, &q);
        const uint32_t unfitted = pl.wf_capacity;
        fit_wavefront(*s, pl);
        mcpt_plan_info r;
        std::memset(&r, 0, sizeof r);
        const bool wf = pl.pipeline == MCPT_PIPELINE_WAVEFRONT;
        r.pipeline = pl.pipeline;
        if (wf) r.variant = pl.route.variant;
        else r.variant = mcpt::megakernel_variant(s->gpu).variant;
        r.wf_streams = wf ? pl.wf_streams : 0;
        r.wf_batch = wf ? pl.wf_capacity : 0;
        r.wf_batch_default = wf ? unfitted : 0;
        r.wf_refill = wf ? pl.wf_refill : 0;
        r.wf_group_shift = wf ? static_cast<int32_t>(pl.route.group_shift) : 0;
        r.ready_thresh = wf ? 0 : pl.kp.ready_thresh;
        r.tail_units = wf ? 0 : static_cast<int32_t>(tail_units_for(*s, pl));
        r.work_paths = pl.work;
        // what prepare_render would hold: partial sums, the small block, the spill areas, queues or tail
        uint64_t ws = uint64_t(pl.kp.nchunks) * pl.kp.npix_local * 16 + sizeof(mcpt::RenderBlock) + spill_bytes(*s, pl.sets());
        if (wf) {
            r.wf_queue_bytes = uint64_t(wf_layout(pl, pl.wf_capacity).need) * uint64_t(pl.wf_streams);
            ws += r.wf_queue_bytes;
        }
        else ws += uint64_t(r.tail_units) * pl.kp.chunk * 16;
        r.workspace_bytes = ws;
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        r.device_free_bytes = fr;
        r.devices = multi ? n : 1;
        r.peer_access = s->peer_access ? 1 : 0;
        *out = r;
        return MCPT_OK;
    });
}

}  // extern "C"
