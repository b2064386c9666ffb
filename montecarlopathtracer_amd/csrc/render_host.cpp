// render_host.cpp -- the render entries of the C ABI (include/mcpt.h): a render
// on one device (RenderScene of the reference's PW::Tracer module,
// CVMCTracer/CUDA/CUTracer.cu:220-404), on several with a peer-copy or RCCL
// gather, its statistics, mcpt_scene_reserve, and the renders built on it: the
// variance, adaptive sampling and the first-hit feature buffers.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>

#include "adaptive_launch.hpp"
#include "aov_launch.hpp"
#include "capi_internal.hpp"
#include "variance_launch.hpp"

using namespace mcpt::host;

namespace mcpt::host {

// the wavefront's streams for a render on st: the caller's, then the scene's side streams
mcpt::WfStreams wf_streams_on(const mcpt_scene& s, int n, hipStream_t st) {
    mcpt::WfStreams wst{};
    wst.n = n;
    wst.st[0] = st;
    wst.fork = s.wf_fork;
    for (int i = 1; i < wst.n; i++) {
        wst.st[i] = s.wf_stream[i];
        wst.join[i] = s.wf_join[i];
    }
    return wst;
}

}  // namespace mcpt::host

namespace {

// RCCL, resolved from librccl at the first render that asks for its gather
// (mcpt_render_params::gather): libmcpt itself does not depend on it, so it
// loads where RCCL is absent and a one-process renderer that never asks pays
// nothing for it.
struct Rccl {
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGather) gather = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    std::string load_error;
};
const Rccl& rccl() {
    static const Rccl r = [] {
        Rccl x;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            const char* e = dlerror();
            x.load_error = std::string("cannot load librccl: ") + (e ? e : "?");
            return x;
        }
        x.comm_init_all = reinterpret_cast<decltype(&ncclCommInitAll)>(dlsym(h, "ncclCommInitAll"));
        x.comm_destroy = reinterpret_cast<decltype(&ncclCommDestroy)>(dlsym(h, "ncclCommDestroy"));
        x.gather = reinterpret_cast<decltype(&ncclGather)>(dlsym(h, "ncclGather"));
        x.group_start = reinterpret_cast<decltype(&ncclGroupStart)>(dlsym(h, "ncclGroupStart"));
        x.group_end = reinterpret_cast<decltype(&ncclGroupEnd)>(dlsym(h, "ncclGroupEnd"));
        x.error_string = reinterpret_cast<decltype(&ncclGetErrorString)>(dlsym(h, "ncclGetErrorString"));
        if (!x.comm_init_all || !x.comm_destroy || !x.gather || !x.group_start || !x.group_end || !x.error_string)
            x.load_error = "librccl lacks ncclCommInitAll / ncclGather / ncclGroupStart / ncclGroupEnd";
        return x;
    }();
    return r;
}

#define NCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess)                                                                          \
            throw mcpt::Error{MCPT_E_DEVICE, std::string(#expr) + ": " + rccl().error_string(r_)};   \
    } while (0)

void render_multi(mcpt_scene& s, const mcpt_render_params* p, float* d_fb, hipStream_t st);

void ensure_capture_timing(mcpt_scene& s) {
    if (s.has_capture_timing) return;
    for (auto& ev : s.capture_timing.e) HIP_TRY(hipEventCreate(&ev));
    s.has_capture_timing = true;
}

// the three events around a render's kernels: the scene's capture events on a
// capturing stream, else a triple off the free list or a new one
Timing acquire_timing(mcpt_scene& s, bool capturing) {
    Timing t;
    if (capturing) {
        ensure_capture_timing(s);
        t = s.capture_timing;
    } else if (!s.free_timing.empty()) {
        t = s.free_timing.back();
        s.free_timing.pop_back();
    } else {
        for (auto& ev : t.e) HIP_TRY(hipEventCreate(&ev));
    }
    return t;
}

// d_var: also the per-pixel variance of this call's pixel mean (variance.hip),
// from the partial sums the render's kernels wrote, behind them on st.
// fitted: the render's plan as it was fitted to memory (one device only)
void render_async(mcpt_scene& s, const mcpt_render_params* p, float* d_fb, hipStream_t st,
                  uint32_t* d_unit_counters = nullptr, bool raw_mean = false, float* d_var = nullptr,
                  Plan* fitted = nullptr) {
    if (!s.on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    if (!d_fb) throw mcpt::Error{MCPT_E_INVALID, "framebuffer is NULL"};
    if (multi_device(s, p, d_unit_counters)) {
        render_multi(s, p, d_fb, st);
        return;
    }
    set_device(s);
    Prepared R;
    prepare_render(s, p, stream_capturing(st), d_unit_counters != nullptr, R);
    Plan& pl = R.pl;
    pl.kp.raw_mean = raw_mean ? 1 : 0;
    pl.kp.unit_counters = d_unit_counters;
    if (fitted) *fitted = pl;
    // (a render without primary lists reports none)
    HIP_TRY(hipMemsetAsync(tile_classes(s), 0, sizeof(mcpt::RenderBlock::tile_classes), st));
    const Timing t = acquire_timing(s, pl.capturing);
    if (pl.pipeline == MCPT_PIPELINE_WAVEFRONT) {
        HIP_TRY(mcpt::launch_wavefront(pl.kp, pl.route, R.wf, wf_streams_on(s, pl.sets(), st), t.e[0], t.e[1], t.e[2],
                                       reinterpret_cast<float4*>(d_fb), &s.last_variant));
    } else {
        HIP_TRY(mcpt::launch_render(pl.kp, s.cus, st, t.e[0], t.e[1], t.e[2], reinterpret_cast<float4*>(d_fb),
                                    &s.last_variant));
    }
    if (d_var) HIP_TRY(mcpt::launch_variance(pl.kp, reinterpret_cast<float4*>(d_var), st));
    if (pl.capturing) return;   // timed and counted when replayed, not now
    s.pending.push_back(t);
    s.renders++;
}

void read_stats(mcpt_scene& s, mcpt_render_stats* out) {
    set_device(s);
    double kms = 0, rms = 0;
    for (auto& t : s.pending) {
        HIP_TRY(hipEventSynchronize(t.e[2]));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, t.e[0], t.e[1]));
        HIP_TRY(hipEventElapsedTime(&b, t.e[1], t.e[2]));
        kms += a;
        rms += b;
        s.free_timing.push_back(t);
    }
    s.pending.clear();
    unsigned long long st[mcpt::kStatSlots] = {};
    if (s.ws.small.p) {
        // the whole record in one copy and one clear (the tile classes behind it are a render's to clear)
        unsigned long long* const d_stats = render_block(s)->stats;
        HIP_TRY(hipMemcpy(st, d_stats, sizeof st, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(d_stats, 0, sizeof st));
        HIP_TRY(hipStreamSynchronize(nullptr));   // (as in prepare_workspace: before a render on a non-blocking stream)
        if (st[mcpt::kStatPhaseUnits] | st[mcpt::kStatPhaseTrav] | st[mcpt::kStatPhaseShade] | st[mcpt::kStatPhaseIters])
            // diagnostic builds (-DMCPT_PHASE_TIMING) only
            std::fprintf(stderr, "mcpt phase cycles (sum over waves): units %llu trav %llu shade %llu burst_iters %llu "
                         "scatter %llu\n", st[mcpt::kStatPhaseUnits], st[mcpt::kStatPhaseTrav], st[mcpt::kStatPhaseShade],
                         st[mcpt::kStatPhaseIters], st[mcpt::kStatPhaseScatter]);
#ifdef MCPT_PHASE_TIMING
        {
            unsigned long long lu[6], lw[6];
            mcpt::read_lane_use(lu);
            mcpt::read_lane_use_wf(lw);
            for (int i = 0; i < 6; i++) lu[i] += lw[i];
            std::fprintf(stderr, "mcpt lane use: descent %.3f (%llu wave-iters) triangle %.3f (%llu) burst %.3f (%llu)\n",
                         lu[0] ? double(lu[1]) / (64.0 * lu[0]) : 0.0, lu[0], lu[2] ? double(lu[3]) / (64.0 * lu[2]) : 0.0,
                         lu[2], lu[4] ? double(lu[5]) / (64.0 * lu[4]) : 0.0, lu[4]);
        }
#endif
    }
    mcpt_render_stats r;
    stats_from_counters(st, r);
    s.routes = RouteCounts{st[mcpt::kStatDirect], st[mcpt::kStatExtend], st[mcpt::kStatClipped], st[mcpt::kStatPrimaryShaded],
                           st[mcpt::kStatSphereSkips]};
    r.renders = s.renders;
    s.renders = 0;
    r.kernel_ms = kms;
    r.reduce_ms = rms;
    r.variant = s.last_variant;
    if (out) *out = r;
}

// Multi-device render (mcpt_init with n > 1; the reference's Initialize(),
// CUTracer.cu:220-223, picked one device): shard r of n = the interleaved tiles
// t with t % n == r (the same partition as the one-process-per-GPU bench),
// rendered by device r into its packed means, peer-copied (xGMI DMA) into the
// primary's gather buffer, then unpermuted there with the running mean.  The
// RNG is keyed per (pixel, sample), so the image is the single-device one bit
// for bit.  Cross-device order: every shard waits for `start` (recorded on the
// caller's stream), the caller's stream waits for every shard's `done`.
// RCCL gather: one communicator per device of the list (ncclCommInitAll,
// rank r = the list's device r), made once per scene
void ensure_comms(mcpt_scene& s) {
    if (!s.comms.empty()) return;
    const Rccl& R = rccl();
    if (!R.load_error.empty()) throw mcpt::Error{MCPT_E_UNSUPPORTED, R.load_error};
    std::vector<int> devs{s.device};
    for (auto& rep : s.replicas) devs.push_back(rep->device);
    std::vector<ncclComm_t> comms(devs.size(), nullptr);
    NCCL_TRY(R.comm_init_all(comms.data(), static_cast<int>(devs.size()), devs.data()));
    s.comms = comms;
}

// packed pixels per shard slot of an n-way multi-device render (>= every shard's count)
uint64_t multi_slot(const Plan& full, const mcpt_render_params* p, int n) {
    const int T = full.kp.tile;
    const uint64_t ntiles = uint64_t(full.kp.tiles_x) * ((uint64_t(p->height) + T - 1) / T);
    return (ntiles + n - 1) / n * uint64_t(T) * uint64_t(T);
}

void render_multi(mcpt_scene& s, const mcpt_render_params* p, float* d_fb, hipStream_t st) {
    DeviceGuard guard;   // an error on a replica's device must not leave that device current
    set_device(s);
    const Plan full = make_plan(s, p);                  // validates p (gather included); row-major output
    const bool use_rccl = p->gather == MCPT_GATHER_RCCL;
    const int n = 1 + static_cast<int>(s.replicas.size());
    const int T = full.kp.tile;
    const uint64_t slot = multi_slot(full, p, n);
    if (slot * n >= (uint64_t(1) << 32)) throw mcpt::Error{MCPT_E_UNSUPPORTED, "image too large"};
    const bool cap = stream_capturing(st);
    grow_ws(s, s.gather, size_t(n) * slot * 16, cap);
    if (use_rccl) {
        ensure_comms(s);
        // every rank sends `slot` pixels (ncclGather's equal counts; the shards'
        // own counts differ by at most one tile): rank 0 from gather_send
        grow_ws(s, s.gather_send, size_t(slot) * 16, cap);
    }
    if (!s.start) HIP_TRY(hipEventCreateWithFlags(&s.start, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s.start, st));
    for (int r = 1; r < n; ++r) {
        mcpt_scene& R = *s.replicas[size_t(r - 1)];
        set_device(R);
        const mcpt_render_params pr = shard_params(*p, n, r);
        const size_t bytes = size_t(mcpt_shard_pixel_count(&pr)) * 16;
        grow_ws(R, R.ws.fb, use_rccl ? size_t(slot) * 16 : bytes, cap);
        HIP_TRY(hipStreamWaitEvent(R.stream, s.start, 0));
        render_async(R, &pr, static_cast<float*>(R.ws.fb.p), R.stream, nullptr, true);
        if (use_rccl) continue;                        // gathered below, all ranks in one group
        char* dst = static_cast<char*>(s.gather.p) + size_t(r) * slot * 16;
        if (!bytes) {
            // a shard that owns no tile: nothing to copy
        } else if (R.device == s.device && !p->force_peer_copy)
            HIP_TRY(hipMemcpyAsync(dst, R.ws.fb.p, bytes, hipMemcpyDeviceToDevice, R.stream));
        else
            HIP_TRY(hipMemcpyPeerAsync(dst, s.device, R.ws.fb.p, R.device, bytes, R.stream));
        HIP_TRY(hipEventRecord(R.done, R.stream));
    }
    set_device(s);
    const mcpt_render_params p0 = shard_params(*p, n, 0);
    render_async(s, &p0, static_cast<float*>(use_rccl ? s.gather_send.p : s.gather.p), st, nullptr, true);
    if (use_rccl) {
        // ncclGather of every rank's `slot` packed pixels into devices[0]'s
        // gather buffer (rank r at r * slot), each on the stream its shard was
        // rendered on; one group, as one process drives every rank
        const Rccl& R = rccl();
        const size_t count = size_t(slot) * 4;
        NCCL_TRY(R.group_start());
        try {
            for (int r = 0; r < n; ++r) {
                const void* send = r ? s.replicas[size_t(r - 1)]->ws.fb.p : s.gather_send.p;
                hipStream_t rs = r ? s.replicas[size_t(r - 1)]->stream : st;
                NCCL_TRY(R.gather(send, r ? nullptr : s.gather.p, count, ncclFloat32, 0, s.comms[size_t(r)], rs));
            }
        } catch (...) {
            (void)R.group_end();
            throw;
        }
        NCCL_TRY(R.group_end());
        for (auto& rep : s.replicas) {
            set_device(*rep);
            HIP_TRY(hipEventRecord(rep->done, rep->stream));
        }
        set_device(s);
    }
    for (auto& R : s.replicas) HIP_TRY(hipStreamWaitEvent(st, R->done, 0));
    mcpt::GatherParams g{};
    g.src = static_cast<const float4*>(s.gather.p);
    g.fb = reinterpret_cast<float4*>(d_fb);
    g.slot = static_cast<uint32_t>(slot);
    g.width = p->width; g.height = p->height; g.tile = T; g.tiles_x = full.kp.tiles_x; g.nshards = n;
    g.prev_count = p->prev_count;
    g.mode = p->mode;
    HIP_TRY(mcpt::launch_gather(g, st));
}

// stats of a (multi-device) scene: counters summed over devices; kernel and
// reduce times the slowest device's (the devices run concurrently)
void read_stats_all(mcpt_scene& s, mcpt_render_stats* out) {
    mcpt_render_stats r;
    read_stats(s, &r);
    for (auto& R : s.replicas) {
        mcpt_render_stats q;
        read_stats(*R, &q);
        r.rays += q.rays; r.paths += q.paths; r.inner_visits += q.inner_visits; r.leaf_visits += q.leaf_visits;
        r.leaf_refs += q.leaf_refs; r.tri_tests += q.tri_tests; r.shades += q.shades;
        r.stack_spills += q.stack_spills;
        s.routes += R->routes;
        r.kernel_ms = std::max(r.kernel_ms, q.kernel_ms);
        r.reduce_ms = std::max(r.reduce_ms, q.reduce_ms);
    }
    r.devices = 1 + static_cast<int32_t>(s.replicas.size());
    set_device(s);
    if (out) *out = r;
}

// What both feature-buffer entries ask of their arguments once each has checked
// its pointers for NULL in its own words
void check_aov(const mcpt_scene& s, const mcpt_render_params* p, const float* ac, const float* nd) {
    if (ac == nd) throw mcpt::Error{MCPT_E_INVALID, "albedo_cov and normal_depth are the same buffer"};
    if (p->width <= 0 || p->height <= 0) throw mcpt::Error{MCPT_E_INVALID, "width/height must be positive"};
    if (p->spp == 0) throw mcpt::Error{MCPT_E_INVALID, "spp must be > 0"};
    if (!s.on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    if (p->shard_count > 1 || p->packed)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "feature buffers are not sharded: shard_count <= 1, packed = 0"};
}

// First-hit feature buffers (aov.hip) of p's frame into two device buffers of
// 4 floats per pixel.  The only workspace is the scene's stack spill area,
// sized by lanes exactly as a render's (grow_spill), so after a render,
// a reserve or a first call nothing is allocated; no counter, event or stats
// record of the scene is touched.
void aov_async(mcpt_scene& s, const mcpt_render_params* p, float* d_ac, float* d_nd, hipStream_t st) {
    if (!p) throw mcpt::Error{MCPT_E_INVALID, "params is NULL"};
    if (!d_ac || !d_nd) throw mcpt::Error{MCPT_E_INVALID, "NULL feature buffer"};
    check_aov(s, p, d_ac, d_nd);
    set_device(s);                        // (a multi-device scene: devices[0], the primary)
    mcpt_render_params q = *p;
    q.spp_chunk = 0;                      // plain sums in sample order
    q.tile = 8;                           // one wave per 8x8 tile
    q.shard_count = 1; q.shard_index = 0;
    q.pipeline = MCPT_PIPELINE_MEGAKERNEL;
    q.max_depth = 0;
    Plan pl = make_plan(s, &q);
    pl.capturing = stream_capturing(st);
    grow_spill(s, 1, pl.capturing);
    pl.kp.spill = static_cast<uint4*>(s.ws.spill.p);
    pl.kp.total_lanes = static_cast<uint32_t>(launched_lanes(s));
    HIP_TRY(mcpt::launch_aov(pl.kp, reinterpret_cast<float4*>(d_ac), reinterpret_cast<float4*>(d_nd), st));
}

// What mcpt_render_var[_device] asks of a render beyond mcpt_render's own
// checks; throws before anything is launched.  The variance is a batch-means
// estimate over the render's chunks, so it needs at least two of them.
void check_var_params(const mcpt_scene& s, const mcpt_render_params* p) {
    if (!p) throw mcpt::Error{MCPT_E_INVALID, "params is NULL"};
    if (p->width <= 0 || p->height <= 0) throw mcpt::Error{MCPT_E_INVALID, "width/height must be positive"};
    if (p->spp == 0) throw mcpt::Error{MCPT_E_INVALID, "spp must be > 0"};
    if (p->spp_chunk == 0 || p->spp_chunk >= p->spp)
        throw mcpt::Error{MCPT_E_INVALID, "the variance needs at least two chunks: set spp_chunk to 1 .. spp - 1 "
                                          "(spp_chunk = 0 is one chunk)"};
    if (p->shard_count > 1 || p->packed)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "the variance is not sharded: shard_count <= 1, packed = 0"};
    if (!s.replicas.empty() || p->gather == MCPT_GATHER_RCCL)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "the variance needs a one-device scene and the peer gather"};
}
void check_var_render(const mcpt_scene& s, const mcpt_render_params* p) {
    check_var_params(s, p);
    if (!s.on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
}

// mcpt_adaptive_params with every default resolved (NULL: all defaults)
struct Adaptive {
    int32_t max_passes, min_passes, radius;
    float threshold, lum_floor;
    bool force_list;
};
Adaptive adaptive_resolve(const mcpt_adaptive_params* p) {
    mcpt_adaptive_params z;
    std::memset(&z, 0, sizeof z);
    if (!p) p = &z;
    if (p->max_passes < 0 || p->max_passes > 4096)
        throw mcpt::Error{MCPT_E_INVALID, "max_passes must be 0 (default 8) or 1..4096"};
    Adaptive a;
    a.max_passes = p->max_passes ? p->max_passes : 8;
    if (p->min_passes < 0 || p->min_passes > a.max_passes)
        throw mcpt::Error{MCPT_E_INVALID, "min_passes must be 0 (default 1) or 1..max_passes"};
    a.min_passes = p->min_passes ? p->min_passes : 1;
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold))
        throw mcpt::Error{MCPT_E_INVALID, "threshold must be finite and >= 0 (0 = default 0.2)"};
    a.threshold = p->threshold != 0.0f ? p->threshold : 0.2f;
    if (!(p->lum_floor >= 0.0f) || !std::isfinite(p->lum_floor))
        throw mcpt::Error{MCPT_E_INVALID, "lum_floor must be finite and >= 0 (0 = default 0.01)"};
    a.lum_floor = p->lum_floor != 0.0f ? p->lum_floor : 0.01f;
    if (p->dilate > 4) throw mcpt::Error{MCPT_E_INVALID, "dilate must be at most 4 (0 = default 1, < 0 = none)"};
    a.radius = p->dilate == 0 ? 1 : (p->dilate < 0 ? 0 : p->dilate);
    if (p->force_list != 0 && p->force_list != 1) throw mcpt::Error{MCPT_E_INVALID, "force_list must be 0 or 1"};
    a.force_list = p->force_list == 1;
    return a;
}

// What mcpt_render_adaptive[_device] asks beyond mcpt_render_var; throws
// before anything is launched.  any_pipeline: the _ex entries, which honour
// p->pipeline; the older pair is the megakernel-only form.
void check_adaptive_render(const mcpt_scene& s, const mcpt_render_params* p, const Adaptive& a, hipStream_t st,
                           bool any_pipeline) {
    check_var_params(s, p);
    (void)make_plan(s, p);   // mcpt_render's own argument checks
    if (p->prev_count != 0)
        throw mcpt::Error{MCPT_E_INVALID, "prev_count must be 0: an adaptive render starts its own running mean"};
    if (uint64_t(p->spp_offset) + uint64_t(a.max_passes) * uint64_t(p->spp) > (uint64_t(1) << 32))
        throw mcpt::Error{MCPT_E_INVALID, "spp_offset + max_passes * spp passes 2^32 sample indices"};
    if (!any_pipeline && p->pipeline != MCPT_PIPELINE_MEGAKERNEL)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "pipeline: adaptive sampling runs on the megakernel only"};
    if (p->mode != MCPT_MODE_CVMCTRACER)
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "mode: adaptive sampling selects in linear radiance, CVMCTracer mode only"};
    if (!s.on_device) throw mcpt::Error{MCPT_E_INVALID, "scene was created host-only"};
    if (stream_capturing(st))
        throw mcpt::Error{MCPT_E_UNSUPPORTED, "hip_stream is capturing a graph: the host reads the pixel list's "
                                              "length each pass"};
}

// The passes of an adaptive render on st (arguments checked).  The host waits
// for st once per listed pass, for the list's length; the last pass is left
// running.  The wavefront (p->pipeline) runs a listed pass as a frame of n listed
// pixels too: wf_generate_list fills an explicit queue 0 and every later kernel
// is the uniform render's, planned inside pass 0's workspace
// (prepare_wavefront_list); the merge stands where its reduction would.
void adaptive_async(mcpt_scene& s, const mcpt_render_params* p, const Adaptive& a, float* d_fb, float* d_var,
                    uint32_t* d_count, hipStream_t st) {
    set_device(s);
    const Plan full = make_plan(s, p);
    const size_t npx = size_t(p->width) * size_t(p->height);
    const uint32_t npix = full.kp.npix_local, nb = mcpt::adaptive_blocks(npix);
    mcpt::AdaptiveWs aw{};
    if (a.max_passes > 1) {
        const size_t counts = (size_t(nb) + 1 + 1) / 2 * 8;   // nb + 1 words, the ballots 8-B aligned behind them
        grow_ws(s, s.ad_list, size_t(npix) * 4, false);
        grow_ws(s, s.ad_flags, npx * 4, false);
        grow_ws(s, s.ad_blocks, counts + size_t(nb) * (mcpt::kAdaptiveBlock / 64) * 8, false);
        if (!s.ad_host_n) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.ad_host_n), 64, hipHostMallocDefault));
        aw.list = static_cast<uint32_t*>(s.ad_list.p);
        aw.flags = static_cast<uint32_t*>(s.ad_flags.p);
        aw.blocks = static_cast<uint32_t*>(s.ad_blocks.p);
        aw.masks = reinterpret_cast<unsigned long long*>(static_cast<char*>(s.ad_blocks.p) + counts);
    }
    float4* fb = reinterpret_cast<float4*>(d_fb);
    float4* var = reinterpret_cast<float4*>(d_var);
    const bool wavefront = p->pipeline == MCPT_PIPELINE_WAVEFRONT;
    Plan pass0;
    render_async(s, p, d_fb, st, nullptr, false, d_var, &pass0);   // pass 0: every pixel
    HIP_TRY(mcpt::launch_adaptive_fill(d_count, npx, 1u, st));
    for (int32_t j = 1; j < a.max_passes; ++j) {
        mcpt_render_params pj = *p;
        pj.spp_offset = p->spp_offset + uint32_t(j) * p->spp;
        pj.prev_count = uint32_t(j);
        const bool all = j < a.min_passes;
        if (all && !a.force_list) {   // a uniform pass as it is
            render_async(s, &pj, d_fb, st, nullptr, false, d_var);
            HIP_TRY(mcpt::launch_adaptive_fill(d_count, npx, uint32_t(j) + 1u, st));
            continue;
        }
        mcpt::AdaptiveSelect sel;
        sel.threshold = a.threshold;
        sel.lum_floor = a.lum_floor;
        sel.radius = a.radius;
        sel.pass = uint32_t(j);
        sel.all = all ? 1 : 0;
        HIP_TRY(mcpt::launch_adaptive_select(full.kp, sel, aw, fb, var, d_count, st));
        HIP_TRY(hipMemcpyAsync(s.ad_host_n, aw.blocks + nb, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t n = *s.ad_host_n;
        if (!n) break;
        if (n > npix) throw mcpt::Error{MCPT_E_DEVICE, "adaptive pixel list longer than the frame"};
        Prepared R;
        R.pl = make_plan(s, &pj);
        mcpt::KernelParams& k = R.pl.kp;
        Timing t;
        if (wavefront) {
            prepare_wavefront_list(s, R.pl, pass0, n, &pj, R.wf);
            k.pixel_list = aw.list;
            // (a listed pass uses no primary lists: the scene reports no tile classes after it)
            HIP_TRY(hipMemsetAsync(tile_classes(s), 0, sizeof(mcpt::RenderBlock::tile_classes), st));
            t = acquire_timing(s, false);
            HIP_TRY(mcpt::launch_wavefront(k, R.pl.route, R.wf, wf_streams_on(s, R.pl.sets(), st), t.e[0], t.e[1],
                                           nullptr, nullptr, &s.last_variant));
        } else {
            // a frame of n listed pixels: the unit decode, tail split and partial-sum
            // layout are the megakernel's own, over n pixels instead of npix_local
            k.npix_local = n;
            k.total_units = n * k.nchunks;
            k.div_npix = mcpt::FastDiv::make(n);
            prepare_workspace(s, R.pl, true);
            k.pixel_list = aw.list;
            t = acquire_timing(s, false);
            HIP_TRY(mcpt::launch_render_list(k, s.cus, st, t.e[0], t.e[1], &s.last_variant));
        }
        HIP_TRY(mcpt::launch_adaptive_merge(k, fb, var, d_count, st));
        HIP_TRY(hipEventRecord(t.e[2], st));
        s.pending.push_back(t);
        s.renders++;
    }
}

// var_rgba: mcpt_render_var -- the variance buffer (4 floats per pixel) is
// staged behind the framebuffer in the scene's host-render buffer
int render_sync(mcpt_scene* s, const mcpt_render_params* p, float* fb_rgb, mcpt_render_stats* stats,
                uint32_t* unit_counters, float* var_rgba = nullptr) {
    return guarded([&]() -> int {
        if (!s || !fb_rgb) return fail(MCPT_E_INVALID, "NULL argument");
        if (var_rgba) check_var_render(*s, p);
        if (!s->on_device) return fail(MCPT_E_INVALID, "scene was created host-only");
        set_device(*s);
        Plan pl = make_plan(*s, p);
        const size_t npx = pl.out_pixels;
        const auto c = carve({npx * 16, var_rgba ? npx * 16 : size_t(0)});
        ensure_buf(s->ws.fb, c.total);
        float* d_fb = c.at<float>(s->ws.fb.p, 0);
        float* d_var = var_rgba ? c.at<float>(s->ws.fb.p, 1) : nullptr;
        if (var_rgba && p->prev_count > 0) HIP_TRY(hipMemcpy(d_var, var_rgba, npx * 16, hipMemcpyHostToDevice));
        std::vector<float> rgba(npx * 4, 0.0f);
        if (p->prev_count > 0) {
            rgb_to_rgba(fb_rgb, npx, rgba.data());
            HIP_TRY(hipMemcpy(d_fb, rgba.data(), npx * 16, hipMemcpyHostToDevice));
        } else {
            HIP_TRY(hipMemset(d_fb, 0, npx * 16));
        }
        read_stats_all(*s, nullptr);   // start a fresh record
        TempDev uc;
        const size_t uc_bytes = size_t(pl.kp.total_units) * 16;
        if (unit_counters) {
            uc.alloc(uc_bytes);
            HIP_TRY(hipMemset(uc.p, 0, uc_bytes ? uc_bytes : 16));
        }
        render_async(*s, p, d_fb, nullptr, static_cast<uint32_t*>(uc.p), false, d_var);
        HIP_TRY(hipStreamSynchronize(nullptr));
        if (var_rgba) HIP_TRY(hipMemcpy(var_rgba, d_var, npx * 16, hipMemcpyDeviceToHost));
        if (unit_counters) HIP_TRY(hipMemcpy(unit_counters, uc.p, uc_bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(rgba.data(), d_fb, npx * 16, hipMemcpyDeviceToHost));
        rgba_to_rgb(rgba.data(), npx, fb_rgb);
        read_stats_all(*s, stats);
        return MCPT_OK;
    });
}

}  // namespace

namespace mcpt::host {

// (a scene's destructor: no collective in flight on any device, then the comms)
void destroy_comms(mcpt_scene& s) {
    if (s.comms.empty()) return;
    for (auto& R : s.replicas) {
        (void)hipSetDevice(R->device);
        (void)hipDeviceSynchronize();
    }
    for (ncclComm_t c : s.comms) (void)rccl().comm_destroy(c);
    (void)hipSetDevice(s.device);
}

}  // namespace mcpt::host

extern "C" {

int mcpt_render_device(mcpt_scene* s, const mcpt_render_params* p, float* d_fb_rgba, void* hip_stream) {
    return guarded([&]() -> int {
        if (!s) return fail(MCPT_E_INVALID, "NULL scene");
        render_async(*s, p, d_fb_rgba, static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

int mcpt_render_stats_read(mcpt_scene* s, mcpt_render_stats* out) {
    return guarded([&]() -> int {
        if (!s || !s->on_device) return fail(MCPT_E_INVALID, "scene is not on a device");
        read_stats_all(*s, out);
        return MCPT_OK;
    });
}

int mcpt_render(mcpt_scene* s, const mcpt_render_params* p, float* fb_rgb, mcpt_render_stats* stats) {
    return render_sync(s, p, fb_rgb, stats, nullptr);
}

int mcpt_render_unit_counters(mcpt_scene* s, const mcpt_render_params* p, float* fb_rgb, uint32_t* unit_counters) {
    if (!unit_counters) return fail(MCPT_E_INVALID, "unit_counters is NULL");
    return render_sync(s, p, fb_rgb, nullptr, unit_counters);
}

int mcpt_scene_reserve(mcpt_scene* s, const mcpt_render_params* p) {
    return guarded([&]() -> int {
        if (!s || !s->on_device) return fail(MCPT_E_INVALID, "scene is not on a device");
        DeviceGuard guard;
        // what render_async's prepare_render would allocate for q (the render
        // without unit counters), and what is the reserve's own
        auto reserve = [&](mcpt_scene& sc, const mcpt_render_params* q) {
            set_device(sc);
            sc.reserved = true;
            ensure_capture_timing(sc);   // (events exist before any capture)
            Prepared R;
            prepare_render(sc, q, false, false, R);
            if (R.pl.pipeline == MCPT_PIPELINE_WAVEFRONT) sc.wf_reserved = std::max(sc.wf_reserved, sc.ws.wf.bytes);
        };
        if (!multi_device(*s, p, nullptr)) {
            reserve(*s, p);
            return MCPT_OK;
        }
        const int n = 1 + static_cast<int>(s->replicas.size());
        const bool use_rccl = p->gather == MCPT_GATHER_RCCL;
        set_device(*s);
        const uint64_t slot = multi_slot(make_plan(*s, p), p, n);
        for (int r = 0; r < n; ++r) {
            const mcpt_render_params pr = shard_params(*p, n, r);
            mcpt_scene& sc = r ? *s->replicas[size_t(r - 1)] : *s;
            reserve(sc, &pr);
            if (r) ensure_buf(sc.ws.fb, use_rccl ? size_t(slot) * 16 : size_t(mcpt_shard_pixel_count(&pr)) * 16);
        }
        set_device(*s);
        // the gather buffer: n slots of the largest shard (shard 0 owns the most tiles)
        ensure_buf(s->gather, size_t(n) * size_t(slot) * 16);
        if (use_rccl) {   // the communicators and rank 0's send buffer exist before any capture
            ensure_comms(*s);
            ensure_buf(s->gather_send, size_t(slot) * 16);
        }
        if (!s->start) HIP_TRY(hipEventCreateWithFlags(&s->start, hipEventDisableTiming));
        return MCPT_OK;
    });
}

int mcpt_render_aov_device(mcpt_scene* s, const mcpt_render_params* p, float* d_albedo_cov, float* d_normal_depth,
                           void* hip_stream) {
    return guarded([&]() -> int {
        if (!s) return fail(MCPT_E_INVALID, "NULL scene");
        aov_async(*s, p, d_albedo_cov, d_normal_depth, static_cast<hipStream_t>(hip_stream));
        return MCPT_OK;
    });
}

int mcpt_render_aov(mcpt_scene* s, const mcpt_render_params* p, float* albedo_cov, float* normal_depth) {
    return guarded([&]() -> int {
        if (!s || !p || !albedo_cov || !normal_depth) return fail(MCPT_E_INVALID, "NULL argument");
        check_aov(*s, p, albedo_cov, normal_depth);
        set_device(*s);
        // staging: both buffers in the scene's host-render framebuffer
        const size_t bytes = size_t(p->width) * size_t(p->height) * 16;
        const auto c = carve({bytes, bytes});
        ensure_buf(s->ws.fb, c.total);
        float* d_ac = c.at<float>(s->ws.fb.p, 0);
        float* d_nd = c.at<float>(s->ws.fb.p, 1);
        if (p->prev_count > 0) {
            HIP_TRY(hipMemcpy(d_ac, albedo_cov, bytes, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_nd, normal_depth, bytes, hipMemcpyHostToDevice));
        }
        aov_async(*s, p, d_ac, d_nd, nullptr);
        HIP_TRY(hipStreamSynchronize(nullptr));
        HIP_TRY(hipMemcpy(albedo_cov, d_ac, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(normal_depth, d_nd, bytes, hipMemcpyDeviceToHost));
        return MCPT_OK;
    });
}

int mcpt_render_var_device(mcpt_scene* s, const mcpt_render_params* p, float* d_fb_rgba, float* d_var_rgba,
                           void* hip_stream) {
    return guarded([&]() -> int {
        if (!s) return fail(MCPT_E_INVALID, "NULL scene");
        if (!d_fb_rgba || !d_var_rgba) return fail(MCPT_E_INVALID, "NULL framebuffer or variance buffer");
        if (p && p->width > 0 && p->height > 0) {
            const size_t bytes = size_t(p->width) * size_t(p->height) * 16;
            if (ranges_overlap(d_fb_rgba, bytes, d_var_rgba, bytes))
                return fail(MCPT_E_INVALID, "the framebuffer and the variance buffer overlap");
        }
        check_var_render(*s, p);
        render_async(*s, p, d_fb_rgba, static_cast<hipStream_t>(hip_stream), nullptr, false, d_var_rgba);
        return MCPT_OK;
    });
}

int mcpt_render_var(mcpt_scene* s, const mcpt_render_params* p, float* fb_rgb, float* var_rgba,
                    mcpt_render_stats* stats) {
    if (!var_rgba) return fail(MCPT_E_INVALID, "NULL argument");
    return render_sync(s, p, fb_rgb, stats, nullptr, var_rgba);
}

// the adaptive entries' shared bodies; any_pipeline: the _ex pair (check_adaptive_render)
namespace {

int adaptive_device_entry(mcpt_scene* s, const mcpt_render_params* p, const mcpt_adaptive_params* ap,
                          float* d_fb_rgba, float* d_var_rgba, uint32_t* d_pass_count, void* hip_stream,
                          bool any_pipeline) {
    return guarded([&]() -> int {
        if (!s) return fail(MCPT_E_INVALID, "NULL scene");
        if (!d_fb_rgba || !d_var_rgba || !d_pass_count)
            return fail(MCPT_E_INVALID, "NULL framebuffer, variance buffer or pass-count buffer");
        if (p && p->width > 0 && p->height > 0) {
            const size_t px = size_t(p->width) * size_t(p->height);
            if (ranges_overlap(d_fb_rgba, px * 16, d_var_rgba, px * 16) ||
                ranges_overlap(d_fb_rgba, px * 16, d_pass_count, px * 4) ||
                ranges_overlap(d_var_rgba, px * 16, d_pass_count, px * 4))
                return fail(MCPT_E_INVALID, "the framebuffer, the variance buffer and the pass-count buffer overlap");
        }
        const Adaptive a = adaptive_resolve(ap);
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        check_adaptive_render(*s, p, a, st, any_pipeline);
        adaptive_async(*s, p, a, d_fb_rgba, d_var_rgba, d_pass_count, st);
        return MCPT_OK;
    });
}

// fb, var and the pass counts are staged in the scene's host-render buffer
int adaptive_host_entry(mcpt_scene* s, const mcpt_render_params* p, const mcpt_adaptive_params* ap, float* fb_rgb,
                        float* var_rgba, uint32_t* pass_count, mcpt_render_stats* stats, bool any_pipeline) {
    return guarded([&]() -> int {
        if (!s || !fb_rgb || !var_rgba || !pass_count) return fail(MCPT_E_INVALID, "NULL argument");
        const Adaptive a = adaptive_resolve(ap);
        check_adaptive_render(*s, p, a, nullptr, any_pipeline);
        set_device(*s);
        const size_t npx = size_t(p->width) * size_t(p->height);
        const auto c = carve({npx * 16, npx * 16, npx * 4});
        ensure_buf(s->ws.fb, c.total);
        float* d_fb = c.at<float>(s->ws.fb.p, 0);
        float* d_var = c.at<float>(s->ws.fb.p, 1);
        uint32_t* d_count = c.at<uint32_t>(s->ws.fb.p, 2);
        read_stats_all(*s, nullptr);   // start a fresh record
        adaptive_async(*s, p, a, d_fb, d_var, d_count, nullptr);
        HIP_TRY(hipStreamSynchronize(nullptr));
        std::vector<float> rgba(npx * 4);
        HIP_TRY(hipMemcpy(rgba.data(), d_fb, npx * 16, hipMemcpyDeviceToHost));
        rgba_to_rgb(rgba.data(), npx, fb_rgb);
        HIP_TRY(hipMemcpy(var_rgba, d_var, npx * 16, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(pass_count, d_count, npx * 4, hipMemcpyDeviceToHost));
        read_stats_all(*s, stats);
        return MCPT_OK;
    });
}

}  // namespace

int mcpt_render_adaptive_device(mcpt_scene* s, const mcpt_render_params* p, const mcpt_adaptive_params* ap,
                                float* d_fb_rgba, float* d_var_rgba, uint32_t* d_pass_count, void* hip_stream) {
    return adaptive_device_entry(s, p, ap, d_fb_rgba, d_var_rgba, d_pass_count, hip_stream, false);
}

int mcpt_render_adaptive(mcpt_scene* s, const mcpt_render_params* p, const mcpt_adaptive_params* ap, float* fb_rgb,
                         float* var_rgba, uint32_t* pass_count, mcpt_render_stats* stats) {
    return adaptive_host_entry(s, p, ap, fb_rgb, var_rgba, pass_count, stats, false);
}

int mcpt_render_adaptive_ex_device(mcpt_scene* s, const mcpt_render_params* p, const mcpt_adaptive_params* ap,
                                   float* d_fb_rgba, float* d_var_rgba, uint32_t* d_pass_count, void* hip_stream) {
    return adaptive_device_entry(s, p, ap, d_fb_rgba, d_var_rgba, d_pass_count, hip_stream, true);
}

int mcpt_render_adaptive_ex(mcpt_scene* s, const mcpt_render_params* p, const mcpt_adaptive_params* ap, float* fb_rgb,
                            float* var_rgba, uint32_t* pass_count, mcpt_render_stats* stats) {
    return adaptive_host_entry(s, p, ap, fb_rgb, var_rgba, pass_count, stats, true);
}

}  // extern "C"
