// capi_internal.hpp -- what the host translation units of the C ABI share
// (include/mcpt.h): the opaque handles, the render plan and workspace, the error
// plumbing and the functions one unit defines and another calls.
//   capi.cpp          init, errors, parameter defaults, the denoisers, temporal accumulation
//   scene_image.cpp   models, the device image, scene creation and teardown
//   plan.cpp          the render plan, its workspace, mcpt_plan_query, shards
//   render_host.cpp   renders: one device, several, reserve, variance, adaptive, feature buffers
//   queries.cpp       ray, radiance, ambient-occlusion and direct-lighting queries
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is loaded on first use (render_host.cpp rccl())

#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mcpt.h"
#include "host_model.hpp"
#include "render_launch.hpp"
#include "staging.hpp"
#include "wf_route.hpp"

struct mcpt_model {
    mcpt::ObjModel m;
};

namespace mcpt::host {

// the calling thread's last error (mcpt_last_error); returns code
int fail(int code, const std::string& msg);
// mcpt_init's device list for scenes created later on this thread (empty: the
// current device only), and whether peer access is enabled between every pair
// of its distinct devices
extern thread_local std::vector<int> g_devices;
extern thread_local bool g_peer_ok;

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            throw mcpt::Error{e_ == hipErrorOutOfMemory ? MCPT_E_NOMEM : MCPT_E_DEVICE,   \
                              std::string(#expr) + ": " + hipGetErrorString(e_)};       \
    } while (0)

template <typename F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const mcpt::Error& e) {
        return fail(e.code, e.msg);
    } catch (const std::bad_alloc&) {
        return fail(MCPT_E_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
        return fail(MCPT_E_INVALID, e.what());
    }
}

// a device allocation a scene owns, and how much of it there is
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// a device allocation freed on every exit path unless released to an owner
struct TempDev {
    void* p = nullptr;
    TempDev() = default;
    explicit TempDev(size_t bytes) { alloc(bytes); }
    TempDev(const TempDev&) = delete;
    TempDev& operator=(const TempDev&) = delete;
    ~TempDev() {
        if (p) (void)hipFree(p);
    }
    void alloc(size_t bytes) { HIP_TRY(hipMalloc(&p, bytes ? bytes : 16)); }
    void* release() {
        void* q = p;
        p = nullptr;
        return q;
    }
};

struct Workspace {
    DevBuf partial;
    DevBuf small;        // one mcpt::RenderBlock (stat_blocks.hpp): work-unit counter, stats, tile classes
    DevBuf spill;
    DevBuf fb;           // mcpt_render staging framebuffer
    DevBuf wf;           // wavefront queues / path state (one allocation)
    DevBuf tail;         // megakernel tail split: one float4 per tail sample
};

struct Timing {
    hipEvent_t e[3];
};

// What build_image's scene gives the wavefront's routes (route_tables, scene_image.cpp,
// fills it from the host scene and the image's triangle order; a replica copies the
// primary's whole).  A new table is a member here and its lines in route_tables
struct RouteTables {
    // terminal cull: emitter boxes as box_hit reads them (fp16 rounded outward);
    // n_cull_boxes == 0: the scene does not allow the cull (host_model.hpp)
    uint32_t n_cull_boxes = 0;
    uint32_t cull_box[mcpt::kMaxCullBoxes][3] = {};
    float cull_gain = 0.0f;             // the largest |Kd| or |Ks| component (finite when there are boxes)
    // miss cull: occluder boxes {lo xyz, hi xyz}; n_miss_boxes == 0: none for the scene (host_model.hpp)
    uint32_t n_miss_boxes = 0;
    float miss_box[mcpt::kMaxMissBoxes][6] = {};
    // direct lists: kd id -> its box; triangles per box; the small boxes' counts
    // (4 bits each) and lists as the kernels take them (render_launch.hpp WfParams)
    std::vector<int32_t> tri_box;
    uint32_t box_tris[mcpt::kMaxMissBoxes] = {};
    uint32_t direct_counts = 0;
    uint32_t direct_list[mcpt::kMaxMissBoxes * 16] = {};
    // sphere clip: bit i -- box i has no list and a sphere {centre xyz, radius^2} that
    // cuts something off it (render_launch.hpp "Sphere clip"; host_model.hpp clip_spheres)
    uint32_t clip_spheres = 0;
    float clip_sphere[mcpt::kMaxMissBoxes][4] = {};
};

// The routes a wavefront render's rays took, of the stats record last read (read_stats
// fills it from the kStat* slots of the same names; include/mcpt.h has each accessor's account)
struct RouteCounts {
    uint64_t direct_rays = 0;           // rays resolved from a box's list
    uint64_t extend_rays = 0;           // rays the secondary extends took
    uint64_t clipped_rays = 0;          // of those, the rays an extend started with a selector (clip walk)
    uint64_t primary_shaded = 0;        // paths whose bounce 0 wf_primary_shade shaded
    uint64_t sphere_skips = 0;          // the selected rays a sphere left no walk
    RouteCounts& operator+=(const RouteCounts& o) {
        direct_rays += o.direct_rays;
        extend_rays += o.extend_rays;
        clipped_rays += o.clipped_rays;
        primary_shaded += o.primary_shaded;
        sphere_skips += o.sphere_skips;
        return *this;
    }
};

// Restores the calling thread's current HIP device on every exit path
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace mcpt::host

struct mcpt_scene {
    mcpt::HostScene hs;
    bool on_device = false;
    int device = -1;
    int cus = 0;
    std::vector<unsigned char> image;   // host copy of the device image
    std::vector<uint32_t> tri_order;    // image triangle slot -> kd id
    mcpt::GpuScene gpu{};
    mcpt::host::RouteTables tables;     // the culls' boxes, the direct lists, the clip spheres
    mcpt::host::RouteCounts routes;     // of the stats record last read
    mcpt::host::DevBuf d_image, d_normals;
    mcpt::host::Workspace ws;
    std::vector<mcpt::host::Timing> pending, free_timing;
    // events of renders captured into a graph: recorded by the graph's replays,
    // never read (a captured render has no time of its own) nor recycled
    // (created once, mcpt_scene_reserve)
    mcpt::host::Timing capture_timing{};
    bool has_capture_timing = false;
    int last_variant = 0;
    uint64_t renders = 0;
    // wavefront queue bytes set aside by mcpt_scene_reserve: later renders with a
    // default batch never grow past them (no hipMalloc inside a stream capture)
    size_t wf_reserved = 0;
    // set by mcpt_scene_reserve: from then on a workspace buffer that has to grow
    // is retired (kept until the scene is destroyed), never freed, so a HIP graph
    // captured against the reservation keeps valid pointers (grow_ws)
    bool reserved = false;
    std::vector<void*> retired;
    // multi-device scene (mcpt_init with n > 1): the primary (this object, on
    // devices[0]) owns one replica per further device -- the same image and
    // normals, its own workspace, a non-blocking stream and a completion event --
    // and the gather buffer its shards are peer-copied into
    std::vector<std::unique_ptr<mcpt_scene>> replicas;
    hipStream_t stream = nullptr;       // replicas: the shard's stream
    hipEvent_t done = nullptr;          // replicas: shard rendered and copied
    hipEvent_t start = nullptr;         // primary: inputs ready on the caller's stream
    mcpt::host::DevBuf gather;
    // wavefront: a second stream for every other batch, forked from and joined
    // back into the caller's stream (created on first use)
    hipStream_t wf_stream[mcpt::kMaxWfStreams] = {};   // [0] unused (the caller's)
    hipEvent_t wf_fork = nullptr, wf_join[mcpt::kMaxWfStreams] = {};
    bool peer_access = true;            // multi-device: peer access enabled between every device pair
    // multi-device, gather = RCCL: one communicator per device of the list
    // (ncclCommInitAll, rank r = device r of the list) and rank 0's send buffer
    std::vector<ncclComm_t> comms;
    mcpt::host::DevBuf gather_send;
    // adaptive sampling (mcpt_render_adaptive): the pixel list, the `over` flags,
    // the compaction's block counts and wave ballots, and the pinned word the
    // list's length is copied to each pass
    mcpt::host::DevBuf ad_list, ad_flags, ad_blocks;
    uint32_t* ad_host_n = nullptr;
    // device ray queries (mcpt_trace_device, mcpt_occluded_device): tri_order on
    // the device, and the queries' own counters -- one mcpt::QueryBlocks, the device
    // entries' block (mcpt_trace_stats_read) and the synchronous host entries'
    mcpt::host::DevBuf rq_order, rq_stats;
    // device radiance queries (mcpt_radiance_device): partial sums [chunk][ray],
    // the tail samples and the work-unit counter (kUnitCounterBytes; counters: rq_stats)
    mcpt::host::DevBuf rad_partial, rad_tail, rad_small;
    // their wavefront form (mcpt_radiance_ex_device): one mcpt::WfQueryBlock, the counter
    // block of the query under way and the device entries' route-ray record; and that
    // record as mcpt_trace_stats_read last read it (mcpt_scene_query_route_rays)
    mcpt::host::DevBuf rad_wf_stats;
    uint64_t query_routes[mcpt::kQueryRoutes] = {};
    // ambient-occlusion queries (mcpt_ao_device, mcpt_render_ao_device): one count of
    // unoccluded samples per point or pixel (counters: rq_stats; stacks: ws.spill)
    mcpt::host::DevBuf ao_counts;
    // direct-lighting queries (mcpt_direct_device, mcpt_render_direct_device): the
    // scene's light table (host_model.hpp; built for host-only scenes too), its device
    // copy -- the records of direct_launch.hpp, then the cdf; null without lights --
    // and one float4 per (point or pixel, chunk) of partial sums
    mcpt::LightTable lights;
    mcpt::host::DevBuf d_lights, dl_partial;
    bool dl_prepared = false;           // the kernels' code object is loaded (ensure_direct)

    // every device buffer of the scene: what the destructor frees (a new buffer
    // is declared above and listed here)
    std::vector<mcpt::host::DevBuf*> buffers() {
        return {&d_image, &d_normals, &ws.partial, &ws.small, &ws.spill, &ws.fb, &ws.wf, &ws.tail, &gather, &gather_send,
                &ad_list, &ad_flags, &ad_blocks, &rq_order, &rq_stats, &rad_partial, &rad_tail, &rad_small,
                &rad_wf_stats, &ao_counts, &d_lights, &dl_partial};
    }
    ~mcpt_scene();   // scene_image.cpp
};

namespace mcpt::host {

// the scene's counter blocks on its device (null before the first render / query): addresses only
inline mcpt::RenderBlock* render_block(const mcpt_scene& s) { return static_cast<mcpt::RenderBlock*>(s.ws.small.p); }
inline mcpt::QueryBlocks* query_blocks(const mcpt_scene& s) { return static_cast<mcpt::QueryBlocks*>(s.rq_stats.p); }
inline mcpt::WfQueryBlock* wf_query_block(const mcpt_scene& s) { return static_cast<mcpt::WfQueryBlock*>(s.rad_wf_stats.p); }
// the last render's tile classes (primary lists)
inline uint32_t* tile_classes(const mcpt_scene& s) { return render_block(s)->tile_classes; }

struct Plan {
    mcpt::KernelParams kp;
    size_t out_pixels;
    bool capturing = false;      // the render's stream is capturing a graph: nothing may be allocated
    int pipeline;
    int wf_streams;              // wavefront streams (wavefront_streams)
    uint32_t wf_capacity;        // paths per wavefront batch
    bool wf_batch_explicit;      // the caller asked for this batch (not shrunk to fit memory)
    int32_t wf_sort;             // wavefront material sort (mcpt_render_params::wf_sort)
    int32_t wf_refill;           // idle lanes before an extend wave refills
    mcpt::WfRoute route;         // which steps a wavefront render takes (wf_route.hpp; make_plan)
    int64_t tail_per_lane;       // megakernel tail split: units per lane (< 0 off)
    int64_t tail_exact;          // megakernel tail split: exact units (> 0 overrides)
    uint64_t wf_mem_limit;       // mcpt_render_params::wf_mem_limit
    uint64_t work;               // paths of the render
    // streams whose extends run concurrently: one spill area and one queue set each
    int sets() const { return pipeline == MCPT_PIPELINE_WAVEFRONT ? wf_streams : 1; }
};

// a render planned with its workspace in place (prepare_render): wf[0 .. pl.sets())
// are the wavefront's per-stream parameters, unused by the megakernel
struct Prepared {
    Plan pl;
    mcpt::WfParams wf[mcpt::kMaxWfStreams];
};

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// ---- plan.cpp ---------------------------------------------------------------
void ensure_buf(DevBuf& b, size_t need);
void grow_ws(mcpt_scene& s, DevBuf& b, size_t need, bool capturing);
void set_device(const mcpt_scene& s);
bool stream_capturing(hipStream_t st);
uint32_t tea16(uint32_t v0, uint32_t v1);
int ready_thresh_for(const mcpt_scene& s, int32_t asked);
// lanes the persistent kernels launch on the scene's device: they index the spill area
size_t launched_lanes(const mcpt_scene& s);
// the scene's part of what a wavefront route is computed from (wf_route.hpp)
mcpt::WfFacts scene_facts(const mcpt_scene& s);
constexpr size_t kSpillEntries = 32;   // stack entries per lane (build_image caps the KD depth at 32), 16 B each
constexpr int64_t kTailPerLane = 4;    // the tail split's default units per lane (make_plan)
size_t spill_bytes(const mcpt_scene& s, int sets);
void grow_spill(mcpt_scene& s, int sets, bool capturing);
uint64_t tail_split(uint64_t lanes, int64_t per_lane, int64_t exact, uint32_t total_units, uint32_t chunk);
uint64_t tail_units_for(const mcpt_scene& s, const Plan& pl);
// the camera of p's eye / dir / up / fov_deg / width / height / mode (render_launch.hpp)
mcpt::CameraConsts camera_consts(const mcpt_render_params& p);
Plan make_plan(const mcpt_scene& s, const mcpt_render_params* p);
void plan_wavefront(const mcpt_scene& s, Plan& pl, const mcpt_render_params* p, bool listed);
uint32_t wf_batch_capacity(const mcpt_scene& s, const mcpt_render_params* p, uint64_t work, uint32_t chunk, int nstr);
void prepare_wavefront_list(mcpt_scene& s, Plan& pl, const Plan& pass0, uint32_t n, const mcpt_render_params* p,
                            mcpt::WfParams* out);
void fit_wavefront(const mcpt_scene& s, Plan& pl);
void prepare_wavefront_rays(mcpt_scene& s, const mcpt::KernelParams& k, const mcpt_render_params* p, bool capturing,
                            Prepared& out);
void prepare_workspace(mcpt_scene& s, Plan& pl, bool tail_split = false, int spill_sets = 1);
// the eight Counters of a block as the record's fields of the same names (devices 1, all else 0)
void stats_from_counters(const unsigned long long c[mcpt::kStatCounters], mcpt_render_stats& st);
void prepare_render(mcpt_scene& s, const mcpt_render_params* p, bool capturing, bool unit_counters, Prepared& out);
bool multi_device(const mcpt_scene& s, const mcpt_render_params* p, const uint32_t* d_unit_counters);
mcpt_render_params shard_params(const mcpt_render_params& p, int n, int r);

// ---- render_host.cpp ----------------------------------------------------------
void destroy_comms(mcpt_scene& s);
mcpt::WfStreams wf_streams_on(const mcpt_scene& s, int n, hipStream_t st);

}  // namespace mcpt::host
