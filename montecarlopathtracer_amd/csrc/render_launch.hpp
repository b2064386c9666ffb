// render_launch.hpp -- device scene image layout, kernel parameters, and the
// host side's shared launch helpers: LDS bytes of a workgroup (lds_bytes_*),
// the megakernel's variant choice, launch_dyn_lds.
//
// Scene image (one contiguous device buffer, 16-byte aligned sections; the
// same bytes are copied verbatim into LDS by the in-LDS kernel variant):
//   tris   3 x float4 per KD triangle: (a.xyz, brute-force rank bits),
//          (a-b .xyz, geometry index bits), (a-c .xyz, the ray-independent
//          minor (a-b).y (a-c).z - (a-c).y (a-b).z of det A and det tM)   48 B
//   nodes  uint2 per KD node (BFS), stored one slot late so that every
//          sibling pair (left, left+1; left is odd in BFS order) is one aligned
//          16-B record: inner x = axis<<30 | left child, y = split value bits;
//          leaf x = 3<<30 | first leaf ref, y = count                       8 B
//   leafs  uint32 per leaf reference: the float4 index (3 x slot) of its
//          triangle's record -- also the index of its normals, and the ray's
//          hit id (no multiply on the hot path)                           4 B
//   (scenes too large for LDS: nodes are 48-B sibling-pair records instead,
//          the two node words + both children's KD boxes as 6 x fp16
//          rounded outward; the root's record is GpuScene::root_w)        48 B
//   geoms  GpuGeom per geometry (material of CUTracer.cu:300-308)      64 B
// Shading normals live outside the image (read once per shaded hit):
//   normals 3 x float4 per KD triangle (n0, n1, n2)                    48 B
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stat_blocks.hpp"

namespace mcpt {

constexpr int kLdsBlock = 1024;          // in-LDS variant: one 16-wave workgroup per CU
constexpr int kGlobalBlock = 256;        // global variant
constexpr int kGlobalBlocksPerCu = 4;
// the wavefront extend's segments (workgroups) per CU for global-memory scenes
#ifndef MCPT_WF_GLOBAL_SEGS
#define MCPT_WF_GLOBAL_SEGS 4
#endif
constexpr int kWfGlobalSegsPerCu = MCPT_WF_GLOBAL_SEGS;
constexpr size_t kMaxLds = 160 * 1024;   // gfx950 LDS per CU
// Terminal cull (wavefront, lean CV renders): after max_depth scatters the path
// loop traces once more and adds color * Ka(hit) * illum.  In a scene whose
// non-emitters all have Ka == 0 a terminal ray that cannot reach an emitter
// adds exactly 0, so every ray that misses all emitter boxes is kept from the
// last closest-hit walk (scene01: ~99% of the last bounce's rays, 6.7% of the
// frame's extend time).  Where: the queue-order shade of an LDS scene with
// occluder boxes (WfParams::shade_cull) tests the ray as it makes it, behind its
// miss-box loop, and does not enqueue it; the sorting shade and global-memory
// scenes run wf_cull_terminal (wavefront.hip) on the last queue.  Both go
// through terminal_ray_adds (wf_device.hpp), and the ray stays counted.
constexpr int kMaxCullBoxes = 8;         // emitter geometries a scene may have and keep the cull
// Primary lists (wavefront, lean CV renders of scenes in LDS, 8x8 tiles): which
// triangles the primary rays of a tile can hit depends on the camera, the tile
// and the scene, not on the sample, so wf_tile_candidates (wavefront.hip) lists
// them once per render call -- every triangle not wholly outside one side plane
// of the tile's jitter-grown frustum -- and wf_primary_lists resolves bounce 0
// from the lists: a tile with no candidate needs no ray, one with up to
// kListK tests them two at a time, a longer list keeps the packet walk.  The
// closest hit is the minimum of (t, rank) over the triangles tested, so a
// superset of the triangles a ray can hit gives the walk's hit id, bit for bit.
// candidates a tile's record holds (longer lists: the walk).  C2 frame, ms,
// three runs each: K = 2 222.1-224.2, 4 221.5-223.5, 6 220.8-227.0, 8 229.2-230.2,
// 16 229.3-229.8 (the parent 234.3-234.8; PERFLOG row 175)
#ifndef MCPT_PRIMARY_LIST_K
#define MCPT_PRIMARY_LIST_K 4
#endif
constexpr uint32_t kListK = MCPT_PRIMARY_LIST_K;
// words of a tile's record: the count, kListK triangle record indices and one
// word more (the extend reads its indices in pairs), in whole 16-B units
constexpr uint32_t kListRecWords = (kListK + 2u + 3u) & ~3u;
// The candidate pass scans every triangle for every tile (one wave per tile).
// Scenes whose image fits in LDS hold fewer than 2000 triangles (48-B records
// in at most 96 KB beside the stack), so the bound only guards the scan's cost
// should that limit ever move: above it the render keeps the packet walk.
constexpr uint32_t kListMaxTris = 4096;
// Primary shade (where the primary lists are read and the queue-order shade culls
// and carries, WfParams::shade_cull): the same 8x8 tile of one sample is one wave's
// group in wf_primary_lists and 64 consecutive indices of bounce 0's shade, so
// wf_primary_shade (wavefront_primary_shade.hip) does both -- it resolves the
// group as wf_primary_lists does and its lanes then run the shade's per-item code
// (wf_shade_item.hpp, the one source of the path rule) on the ray they hold: the
// primary ray is made once, t, beta and gamma are the ones test_tri_pair left, the
// material and the direct lists' records come from the LDS scene image, no hit
// id goes through memory, and a tile without a candidate only gets its zeros.
// Continuing rays go to queue 1's head, resolved ones to its tail (shading them
// once more in place needed scratch at 88 VGPRs, PERFLOG row 185), and the kernel writes bounce 1's counters as a shade does;
// bounce 0 has no shade launch.  Every other render keeps the two kernels.
// C2 frame, ms, six alternated runs: 143.6-144.3 -> 135.7-136.6 (PERFLOG row 185).
// Miss cull (wavefront, lean renders): a secondary ray whose segment
// (0, best_init] misses the box of every triangle has no hit; the next shade
// would turn its miss into zero radiance and end the path.  The shade that
// creates such a ray (wf_shade_slots) tests it against the scene's occluder
// boxes (host_model.cpp miss_cull_boxes: at most kMaxMissBoxes fp32 AABBs that
// together hold every triangle), stores the zero itself and does not enqueue
// it: the next queue is shorter, every extend keeps its code.  scene01 is a
// box open towards the camera: about one secondary ray in six leaves through
// the opening.  Counting renders keep the full walk (their visit counters stay
// the oracle's).
// boxes a scene may have: the test costs ~25 VALU instructions per box and ray.
// scene01 on the CPU oracle: 6 / 7 / 8 / 10 / 15 boxes recognise 56 / 66 / 86 /
// 86.5 / 88% of the escaping rays (five walls, the light and two boxes over
// the spheres and the block make 8)
constexpr int kMaxMissBoxes = 8;
// Direct lists (wavefront, lean renders of a scene in LDS with occluder boxes):
// the shade's box test also tells which boxes the new ray's segment hits.  A
// hit the walk could accept lies inside the box its triangle was assigned to
// (host_model.cpp direct_list_assign: every triangle goes to one box that holds
// it), so a ray that hits exactly one box can only hit that box's triangles,
// and the closest hit is the minimum of (t, rank) over the triangles tested:
// when that box is small (1..kDirectK triangles; scene01's five walls hold two
// each) the box's list is tested instead of walking the tree -- same hit id,
// bit for bit.  Such a ray is a direct ray; the shade that makes it also
// resolves it (Direct resolve, below).
// triangles a box may hold and keep its list: the smallest K that loses nothing.
// Priced on the CPU oracle (scripts/price_direct_lists.py,
// profiles/direct_lists/pricing.txt): K = 2, 4 and 8 list the same boxes on
// scene01, scene02 and the 70k mesh -- flat two-triangle walls; the next larger
// boxes hold 12 triangles (the lights) -- so the same rays are direct
#ifndef MCPT_DIRECT_K
#define MCPT_DIRECT_K 2
#endif
constexpr uint32_t kDirectK = MCPT_DIRECT_K;
static_assert(kDirectK >= 1 && kDirectK <= 15, "a box's count is carried in 4 bits");
// (kDirectShift, kDepthMask: below, with the clip walk, whose selector they place)
// the extend's LDS copy of the table: kMaxMissBoxes x kDirectK record indices
// and one 16-B unit more (the leaf branch reads its refs in pairs)
constexpr uint32_t kDirectTableWords = kMaxMissBoxes * kDirectK;
constexpr size_t kDirectLdsBytes = (size_t(kDirectTableWords) * 4 + 16 + 15) & ~size_t(15);
// Direct resolve (where the direct lists are active): the shade that makes a
// direct ray also finds its hit -- begin_ray's root clip and test_tri_pair over
// the box's list, the extend's own operations -- and writes ray and hit id to
// the far end of the segment's next queue: a queue's head [0, queued) holds the
// rays its extend walks, its tail [seg - resolved, seg) the resolved ones, and
// the next shade takes both.  A resolved ray without a hit ends as the miss
// cull's rays do, and one made for the terminal query gets the radiance the
// last shade would store (its hit's emission), so the last queue has no tail
// and the terminal cull sees no resolved ray.  No direct ray reaches an extend.
// Carry (queue-order shade, WfParams::shade_cull): the lane that resolved a ray
// keeps it in registers and shades it in its wave's next loop iteration, up to
// kCarryMax (wf_device.hpp) times in a row, so the ray and its hit id are
// neither written to the tail nor read back; only a chain's last ray goes to a
// queue.  tri_hit_params runs from the triangle records as for any slot: the
// values are the ones the next shade would compute.  Queues then hold rays of
// mixed depths (a carried ray's product sits in queue b+1 with a depth above
// b+1), each ray's depth is its own word's, and later queues get shorter.
// The shade reads the lists' records (at most 16 x 48 B) and their indices from
// a copy in its own LDS, kDirectShadeLds bytes counted beside the co-resident
// extend: the reads are a dependent round trip behind the box test (from the
// L2-resident global image the C2 frame gained 1.2% instead of 5.0%, row 179)
constexpr size_t kDirectShadeLds = size_t(kDirectTableWords) * (48 + 4);
static_assert(kDirectTableWords * 3 <= 256, "the shade's smallest workgroup copies one record part per thread");
// Clip walk (where the direct resolve is active): the rays the secondary extends
// still walk are almost all rays through a large box (scene01: one of the two
// 420-triangle objects, usually with one wall behind it).  The shade's box test
// already knows which boxes the new ray's segment hits; a ray that is not direct
// and hits at least one box without a list and at most one box with a list carries
// that 8-bit box mask as its selector, in the top byte of the {d, depth} word (0:
// the full walk; kNoRay, all ones, stays unique: a depth is < 2^24).  The lean LDS
// extend starts such a ray with the root interval cut to the union of its
// unlisted boxes' slab intervals -- the shade's test again, [min lo * kEpsLo,
// max hi * kEpsHi] -- and tests the listed box's triangles first, through the
// leaf branch; the pop behind the list starts the clipped walk or ends the ray
// by the walk's own rule.  Every triangle is in exactly one box, and one the ray
// can pass tri_accept on lies in a box the ray's slab test passes, with its t
// inside that box's interval: the list plus the leaves the walk reaches inside
// the interval are a superset of what the ray can hit, and the closest hit is
// the minimum of (t, rank) over the triangles tested.
// the selector's place in the depth word: the box mask in the top byte
constexpr uint32_t kDirectShift = 24, kDepthMask = (1u << kDirectShift) - 1u;
// a ray's depth is at most 3 * max_depth + 1 (QuinEngine), max_depth <= kMaxDepthParam
constexpr int kMaxDepthParam = 1000;
static_assert(3u * kMaxDepthParam + 1u < kDepthMask, "a ray's depth must fit under its selector");
static_assert(kMaxMissBoxes <= 8, "the clip walk's selector is one byte of box bits");
// (what the shades and extends count of all this per render: stat_blocks.hpp, kStatDirect and on)
// Sphere clip (where the clip walk is active and a box without a list has a sphere):
// an object's box is mostly empty at its corners (a tessellated sphere fills 52% of
// its box), and a clipped ray that crosses only a corner still descends the tree to
// find nothing.  The host keeps, per box without a list, a sphere over the vertices
// of the triangles assigned to it (host_model.cpp clip_spheres: centre at the
// box centre, the radius inflated by kSphereMargin), and wf_sphere_clip -- the lean
// LDS extend with this one change -- intersects each unlisted box's slab interval
// with the ray's interval in that box's sphere (sphere_interval, trace_device.hpp)
// before the union: a hit the walk could accept lies on a triangle, hence inside its
// box's sphere, with its t inside the ray's interval there.  Which rays are culled,
// direct, clipped or walked is the shade's decision and does not change; only where a
// clipped ray's walk starts and ends does, and a ray with nothing left starts none.
// The radius' relative margin
constexpr double kSphereMargin = 1.0 / 1024.0;
// a sphere is kept only where the scene's diagonal is at most this many radii: a
// clipped ray's origin lies in the scene, so |centre - o| / R stays below it and
// the fp32 error of sphere_interval stays a small part of the margin
constexpr double kSphereMaxReach = 256.0;

struct GpuGeom {
    float Ka[3], Kd[3], Ks[3];
    float Ns, Tr, Ni;
    uint32_t Ns_u;                       // (PWuint)Ns, Utils.hpp:72 parameter type
    uint32_t pad[3];
};
static_assert(sizeof(GpuGeom) == 64, "GpuGeom layout");

struct GpuScene {
    const unsigned char* image;
    const float4* normals;
    uint32_t image_bytes;
    uint32_t off_tris, off_nodes, off_leafs, off_geoms;
    uint32_t node_boxes;                 // 1: 48-B pair records with child boxes (global-memory scenes)
    uint32_t n_tris, n_nodes, n_leafs, n_geoms;
    float root_min[3], root_max[3];
    uint32_t root_w[2];                  // root node record (nodes[0])
};

// Unsigned division by a launch-invariant divisor d >= 1 as multiply-high and
// shifts (Granlund & Montgomery 1994, fig. 4.1): exact for every 32-bit n.
// The work-unit decode divides four times per unit; hardware has no integer
// divide, and the generic sequence cost ~5% of C2 at 8-sample chunks.
struct FastDiv {
    uint32_t m, s1, s2, d;
    static FastDiv make(uint32_t d) {
        uint32_t l = 0;
        while (l < 32 && (uint64_t(1) << l) < d) l++;          // ceil(log2 d)
        FastDiv f;
        f.m = static_cast<uint32_t>(((uint64_t(1) << 32) * ((uint64_t(1) << l) - d)) / d + 1);
        f.s1 = l < 1 ? l : 1;
        f.s2 = l > 0 ? l - 1 : 0;
        f.d = d;
        return f;
    }
    __host__ __device__ __forceinline__ uint32_t div(uint32_t n) const {
        const uint32_t t = static_cast<uint32_t>((uint64_t(m) * n) >> 32);   // v_mul_hi_u32
        return (t + ((n - t) >> s1)) >> s2;
    }
};

// One frame's camera as the kernels take it (capi_internal.hpp camera_consts): eye,
// the normalized basis, tan(fov / 2) and -- QuinEngine mode only, else 0 -- the
// projection's two scales
struct CameraConsts {
    float eye[3], fwd[3], up[3], right[3];
    float tan_half_fov, proj11, proj22;
};

struct KernelParams {
    GpuScene scene;
    int32_t width, height;
    int32_t tile, tiles_x, shard_count, shard_index, packed;
    uint32_t npix_local;                 // owned tiles * tile^2
    uint32_t spp, spp_offset, chunk, nchunks, total_units;
    int32_t max_depth;
    float illum, tan_half_fov;
    int32_t fresnel_kd;
    uint32_t prev_count;
    int32_t mode;                        // 0 CVMCTracer, 1 QuinEngine (rtx.hlsl:304-405)
    float proj11, proj22;                // QE projection scales (PerspectiveFovRH)
    float best_init;                     // closest-hit start: FLT_MAX, QE 10000 (rtx.hlsl:88)
    float eye[3], fwd[3], up[3], right[3];
    uint32_t key;                        // TEA-16 key of the 64-bit seed
    float4* partial;                     // [nchunks][npix_local]
    uint32_t* counter;                   // work-unit counter (RenderBlock::counter)
    unsigned long long* stats;           // RenderBlock::stats: the slots StatSlot names (stat_blocks.hpp)
    uint4* spill;                        // traversal-stack spill [32][total_lanes]
    uint32_t total_lanes;
    uint32_t* unit_counters;             // optional [total_units][4]: rays, inner, leaf, tests
    int32_t ready_thresh;                // lanes ready before a shading round (1..64)
    int32_t lean;                        // 1: no per-step traversal counters (mcpt_render_params::lean)
    FastDiv div_npix, div_tt, div_tiles_x, div_tile;   // npix_local, tile^2, tiles_x, tile
    // Tail split (megakernel): units [tail_units, total_units) -- the last
    // ~6 per lane -- are handed out one sample at a time (work items
    // tail_units + (u - tail_units) * chunk + j), each sample's radiance going
    // to tail_buf[(u - tail_units) * chunk + j]; the reduction sums them in
    // sample order, so the image is the one of whole units, bit for bit.
    uint32_t tail_units, total_items;
    FastDiv div_chunk;                   // chunk
    float4* tail_buf;
    // primary rays (CUTracer.cu:202-203, double): H / W, and 2^-k when W = 2^k (else 0)
    double h_over_w, inv_w_pow2;
    // 1: the reduction writes the plain mean of this call's samples (a device's
    // shard of a multi-device render; gather_kernel applies the running mean)
    int32_t raw_mean;
    // pixel-list kernels (adaptive sampling; the megakernel's list kernel and the
    // wavefront's wf_generate_list): packed pixel index of listed pixel i;
    // npix_local is then the list's length.  To the wavefront's other kernels a non-null
    // pointer only says "queue 0 is explicit" (implicit0, wf_device.hpp): a ray frame sets
    // one that nothing dereferences ("Ray frames" below)
    const uint32_t* pixel_list;
};

// Radiance queries (mcpt_radiance_device, render.hip radiance_kernel): the
// caller's rays, origins / directions as 3 floats each (QueryParams' layout),
// and the optional RNG stream id of each ray (NULL: the ray's index).  A kernel
// argument of its own, behind KernelParams: no field an existing kernel reads moves.
struct RayInputs {
    const float* o;
    const float* d;
    const uint32_t* stream;
};
// Ray frames (the wavefront form of the radiance queries, mcpt_radiance_ex_device): a
// wavefront render of n "pixels" that are the caller's rays, planned as a frame over a
// pixel list is (WfFacts::listed: no packet extend, no primary lists).  wf_ray_generate
// (wavefront_rays.hip) fills an explicit queue 0 from RayInputs as path_body's RAYS form
// starts its paths; bounce 0's extend is wf_ray_extend0, the extend reading its origins
// from the queue; every later kernel is the renders' -- a path is its pid, pid % nb its
// column of the [chunk][ray] partial sums -- and radiance_reduce_kernel ends the frame.
// kp.pixel_list is non-null and never dereferenced; kp.stats is a WfQueryBlock's.
// fewest work items (ray, chunk) a workgroup of the automatic grid gets, so the
// grid shrinks with the work (the ray queries' floor, rayquery_launch.hpp)
constexpr uint32_t kRadMinUnits = 64;

// Multi-device gather (render_host.cpp render_multi): shard r of `nshards` wrote the
// plain means of its owned tiles, packed tile-major, to src[r * slot ...]
// (peer-copied to the primary device); gather_kernel unpermutes them into the
// row-major framebuffer with the running mean of reduce_kernel, bit for bit.
struct GatherParams {
    const float4* src;                   // [nshards][slot]
    float4* fb;                          // row-major W x H
    uint32_t slot;                       // packed pixels per shard slot (>= every shard's count)
    int32_t width, height, tile, tiles_x, nshards;
    uint32_t prev_count;
    int32_t mode;
};

// Closest-hit batch (mcpt_intersect, render.hip query_kernel): rays i < n,
// origins / directions as 3 floats each; out slot[i] = the hit triangle's image
// slot (-1 miss), hit[3i..] = beta, gamma, t; spill = [32][n] stack entries
constexpr int kQueryBlock = 256;
struct QueryParams {
    GpuScene scene;
    const float* o;
    const float* d;
    int32_t* slot;
    float* hit;
    uint4* spill;
    unsigned long long* stats;           // 8 counters (Counters order)
    uint32_t n;
    float best_init;
};

// Wavefront pipeline workspace (wavefront.hip).  One batch = samples
// [s_begin, s_begin + ns) of chunk `chunk` for owned pixels [v0, v0 + nb);
// path id pid = s_local * nb + (v - v0).  The batch is cut into `nseg`
// segments of `seg` paths, one per extend workgroup; a path stays in its
// segment for all bounces, so each segment's queues and counters are private
// to one workgroup (LDS atomics only).  Queue slot j of
// segment g is entry g*seg + j; path state and radiance are indexed by pid.
struct WfCounters {                      // per (bounce, segment), 8 words
    uint32_t queued;                     // rays in this segment's queue (written by its producer)
    uint32_t hits;                       // slots whose hit id extend wrote (= queued; shade's count)
    uint32_t resolved;                   // rays in the queue's tail [seg - resolved, seg), hit ids written by
                                         // the shade that made them
    uint32_t pad[5];
};
struct WfParams {
    // ray queue b: three float4 streams of slot_stride entries (SoA),
    // {o.xyz pid} {d.xyz depth} {throughput.xyz rng}, then the 4-B hit ids;
    // extend reads streams 0-1 and writes the ids, shade reads all four
    float4* q[2];
    float4* radiance;                    // path radiance per pid                   [capacity]
    WfCounters* cnt;                     // [max_depth + 2][nseg]
    uint32_t capacity;                   // paths per batch
    uint32_t slot_stride;                // queue entries per stream (>= nseg * seg)
    uint32_t v0, nb, s_begin, ns, chunk_index;   // pixels [v0, v0+nb) x samples [s_begin, s_begin+ns)
    uint32_t nsc;                        // samples per chunk (ns = whole chunks of nsc)
    uint32_t nseg, seg;                  // segments (= extend workgroups) and slots per segment
    uint32_t group_shift;                // paths are dealt to segments in groups of 2^group_shift
                                         // (the plan's for global-memory scenes; 6 in LDS)
    int32_t bounce;
    int32_t refill_thresh;               // idle lanes before an extend wave refills
    int32_t sort;                        // 1: shade sorts each block of slots by material first
    uint32_t xcd_deal;                   // 1: groups dealt to segments by XCD (global-memory scenes, seg_of)
    // terminal cull: the scene's emitter boxes (one per emitter geometry, fp16
    // rounded outward, packed as box_hit reads them); 0 boxes = no cull.  Last in
    // the kernel arguments, outside the scene image: no offset before them moves
    uint32_t n_cull_boxes;
    uint32_t cull_box[kMaxCullBoxes][3];
    // primary lists: one record of kListRecWords words per owned tile of the
    // call {count, indices}, and the call's tile classes {0, 1..K, > K}
    // (stream 0's are used; also last in the kernel arguments)
    uint32_t* tile_cand;
    uint32_t* tile_classes;
    // miss cull: the scene's occluder boxes {lo xyz, hi xyz} in fp32; 0 boxes =
    // no cull (the scene has none, or a counting render).  Also last in the
    // kernel arguments: only the shade reads them, as scalar operands
    uint32_t n_miss_boxes;
    float miss_box[kMaxMissBoxes][6];
    // direct lists: per occluder box, 4 bits of direct_counts -- the triangles of
    // its list, 0 = the box's rays walk -- and kDirectK words of direct_list, their
    // record indices (the unit of the image's leaf refs) in image order.
    // direct_counts == 0: no ray is direct and none carries a selector (the lists
    // are off for the render: WfRoute::direct, wf_route.hpp).  Behind everything
    // else in the kernel arguments
    uint32_t direct_counts;
    uint32_t direct_list[kDirectTableWords];
    // 1: the queue-order shade owns the terminal cull and carries resolved rays
    // ("Terminal cull", "Direct resolve" above; the route decides per render,
    // WfRoute::shade_cull: lean, scene in LDS with occluder boxes, wf_sort = 0).
    // The last kernel argument: no offset an extend reads moves
    uint32_t shade_cull;
};
// Sphere clip ("Sphere clip" above): bit i of mask -- occluder box i has no list and a
// sphere {centre xyz, radius^2} over its triangles that cuts something off the box.
// wf_sphere_clip's third kernel argument, read as scalar operands: a kernel argument
// of its own behind WfParams, so no argument an existing kernel reads moves or grows
struct SphereClip {
    uint32_t mask;
    float sphere[kMaxMissBoxes][4];
};

// LDS need of the in-LDS variant for a scene image of `image_bytes`: the
// stack's S entries per lane, then the image
inline size_t lds_bytes_in_lds(uint32_t image_bytes, int S) { return (size_t)image_bytes + (size_t)S * kLdsBlock * 16; }
// The persistent kernels that hand out slots from an LDS counter (wavefront
// extends, ray queries) keep it behind the stack and the image, in a 32-B block:
// LDS bytes of such a workgroup with the scene in LDS, and with it in global memory
constexpr size_t kLdsCounterBytes = 32;
inline size_t lds_bytes_counted_in_lds(uint32_t image_bytes, int S) {
    return lds_bytes_in_lds(image_bytes, S) + kLdsCounterBytes;
}
constexpr size_t lds_bytes_global(int S, bool counted) {
    return (size_t)S * kGlobalBlock * 16 + (counted ? kLdsCounterBytes : 0);
}
// Where a scene lives.  build_image (scene_image.cpp) alone compares an image's
// size with kMaxLds, and it fills every GpuScene there is (replicas copy the
// primary's; a cached KD tree goes through build_image like a built one): an
// image that does not fit is built with child boxes, so
//   !node_boxes  implies  lds_bytes_counted_in_lds(image_bytes, 4) <= kMaxLds
// and every kernel with S = 4 stack entries per lane, counter block or not,
// has room for an image without them.  No launcher tests the size again.
inline bool scene_in_lds(const GpuScene& sc) { return !sc.node_boxes; }
// the megakernel's variant for a scene (mcpt_render_stats::variant): 1 / 2 the
// image in LDS with S = 8 / 4 stack entries, 3 in global memory (an image built
// with child boxes, or one too large for LDS)
struct MegakernelVariant {
    int variant;
    bool in_lds;
    int S;
};
MegakernelVariant megakernel_variant(const GpuScene& sc);
// lanes the persistent kernels launch for a scene: they index the spill area
int total_lanes_for(const GpuScene& sc, int cus);
#ifdef __HIP__
// a kernel's dynamic LDS limit raised to lds_bytes; then also its launch
template <typename K>
hipError_t set_dyn_lds(K kernel, size_t lds_bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds_bytes);
}
template <typename K, typename... Args>
hipError_t launch_dyn_lds(K kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args&... args) {
    const hipError_t e = set_dyn_lds(kernel, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
    return hipGetLastError();
}
#endif
// memset counter, path kernel (events ev0/ev1 around it), reduce kernel (ev2)
hipError_t launch_render(const KernelParams& kp, int cus, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1,
                         hipEvent_t ev2, float4* fb, int* variant_out);
hipError_t launch_render_list(const KernelParams& kp, int cus, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1,
                              int* variant_out);
hipError_t launch_reduce(const KernelParams& kp, float4* fb, hipStream_t st);
// radiance query: memset counter, radiance kernel over kp.npix_local rays, the
// query's own reduce into out[ray]; workgroups as radiance_grid says
hipError_t prepare_radiance(const GpuScene& sc);
uint32_t radiance_grid(const GpuScene& sc, uint64_t items, int cus, int max_workgroups);
hipError_t launch_radiance(const KernelParams& kp, const RayInputs& ri, int cus, int max_workgroups, float4* out,
                           hipStream_t st);
// the wavefront's kernels a ray frame of this route launches, and wavefront_rays.hip's,
// resolved on the current device (mcpt_scene_reserve_radiance_ex: as prepare_radiance)
struct WfRoute;
hipError_t load_wavefront(const WfRoute& route);
hipError_t load_wavefront_rays();
// the query's reduce alone (a ray frame's, behind the wavefront's batches)
hipError_t launch_radiance_reduce(const KernelParams& kp, float4* out, hipStream_t st);
// wavefront_rays.hip: a wavefront query's counter block (WfQueryBlock::stats) folded into
// the eight counters of a QueryBlocks member and, unless null, the route-ray record
hipError_t launch_wavefront_ray_fold(const unsigned long long* blk, unsigned long long* counters,
                                     unsigned long long* routes, hipStream_t st);
hipError_t launch_gather(const GatherParams& g, hipStream_t st);
hipError_t launch_query(const QueryParams& q, hipStream_t st);
#ifdef MCPT_PHASE_TIMING
void read_lane_use(unsigned long long out[6]);      // diagnostic build only: megakernel
void read_lane_use_wf(unsigned long long out[6]);   // wavefront extend
#endif
// wavefront pipeline: generate / extend / shade per bounce / accumulate per
// batch, then the same reduction (events: ev0 before, ev1 after the batches)
// wavefront streams: batch i runs on stream i mod n (st[0] = the caller's),
// forked from and joined back into st[0] with the events of each extra stream.
// route: the render's (wf_route.hpp), from the plan that filled wf[]; the batches
// of a default-batch render that can use the primary lists are whole tiles.
// kp.pixel_list set (adaptive sampling's listed passes): a frame of kp.npix_local
// listed pixels, CV mode -- wf_generate_list fills an explicit queue 0, bounce 0
// runs the ordinary extend and shade, no candidate pass; fb == nullptr then skips
// the reduction (the caller merges the partial sums, launch_adaptive_merge)
// rays set: a ray frame ("Ray frames" above) -- generate and bounce 0 read *rays, and fb
// is the query's output, written by the radiance queries' reduction
constexpr int kMaxWfStreams = 4;
struct WfStreams {
    int n;
    hipStream_t st[kMaxWfStreams];
    hipEvent_t fork, join[kMaxWfStreams];
};
struct WfRoute;
hipError_t launch_wavefront(const KernelParams& kp, const WfRoute& route, const WfParams* wf, const WfStreams& ws,
                            hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev2, float4* fb, int* variant_out,
                            const RayInputs* rays = nullptr);

}  // namespace mcpt
