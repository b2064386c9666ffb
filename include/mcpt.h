/*
 * mcpt.h -- C ABI of the MI355X Monte Carlo path-tracing core (libmcpt.so).
 *
 * Drop-in boundary for the reference's tracer module, pw1316/MonteCarloPathTracer
 * CVMCTracer/CVMCTracer/CUDA/CUTracer.h:9-12 (namespace PW::Tracer), whose only
 * caller is CVMCTracer/CVMCTracer/main.cpp:16-18,33-35.  Plain C types only:
 * no HIP, torch or C++ types cross this boundary.  Every function returns
 * MCPT_OK (0) or a negative MCPT_E* code; mcpt_last_error() gives a
 * thread-local message for the last failure on the calling thread.
 *
 *   reference                                         this ABI
 *   ObjModel::readObj(path)  ObjReader.cpp:8-161      mcpt_model_read_obj
 *   cudaError_t Initialize() CUTracer.cu:220-223      mcpt_init
 *   cudaError_t CreateGeometry(const ObjModel*)       mcpt_scene_create (+ KD build,
 *                            CUTracer.cu:225-314       QuinEngine/Utils/KDTree.hpp:58-287)
 *   cudaError_t DestroyGeometry() CUTracer.cu:316-338 mcpt_scene_destroy (frees what it allocated)
 *   cudaError_t RenderScene(int sceneID, PWVector3f*) mcpt_render (host framebuffer, synchronous)
 *                            CUTracer.cu:340-404       mcpt_render_device (device buffer, async)
 *
 * Ownership: a model/scene handle is owned by the caller and used from one
 * thread at a time; the scene owns its device copies; framebuffers are
 * caller-owned.  Framebuffer layout = the reference's hostcolor: row-major
 * y*W + x, linear radiance, fp32 RGB (3 floats per pixel) for mcpt_render;
 * RGBA (4 floats per pixel, A unused) for mcpt_render_device.
 */
#ifndef MCPT_H
#define MCPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCPT_ABI_VERSION 9

enum {
    MCPT_OK = 0,
    MCPT_E_INVALID = -1,   /* bad argument                     */
    MCPT_E_IO = -2,        /* file cannot be opened            */
    MCPT_E_PARSE = -3,     /* "Invalid OBJ file!" (ObjReader.cpp:81) */
    MCPT_E_DEVICE = -4,    /* HIP runtime error                */
    MCPT_E_NOMEM = -5,
    MCPT_E_UNSUPPORTED = -6
};

typedef struct mcpt_model mcpt_model;   /* host ObjModel (ObjReader.hpp:37-63)  */
typedef struct mcpt_scene mcpt_scene;   /* device-resident scene + KD tree      */

typedef struct {
    int64_t n_vertices;    /* incl. dummy index 0 (ObjReader.hpp:44) */
    int64_t n_normals;     /* incl. dummy */
    int64_t n_texcoords;   /* incl. dummy */
    int64_t n_triangles;   /* incl. dummy */
    int64_t n_materials;   /* incl. dummy "" material */
    int64_t n_groups;      /* incl. empty ones, std::map order */
} mcpt_model_info;

typedef struct {
    int64_t n_geometries;  /* non-empty groups (CUTracer.cu:278-285) */
    int64_t n_triangles;   /* triangles covered by a geometry range (KD input) */
    int64_t n_nodes;       /* KD nodes, BFS order */
    int64_t n_leaf_refs;   /* total leaf triangle references */
    int64_t kd_depth;      /* deepest node depth (<= 32) */
    int64_t lds_bytes;     /* LDS image size; 0 if the scene is served from global memory */
    int64_t device;        /* HIP device ordinal holding the scene */
    int64_t node_boxes;    /* 1: served from global memory, children culled by their KD boxes */
    int64_t n_devices;     /* devices holding a replica (mcpt_init's list at creation); 0 host-only */
    int64_t kd_build;      /* MCPT_KD_BUILD_* the tree was built with -- ABI 9 */
} mcpt_scene_info;

typedef struct {
    int32_t width, height;      /* full image (IMG_WIDTH/IMG_HEIGHT, CV/stdafx.h:41-42) */
    uint32_t spp;               /* samples per pixel this call (NUM_SAMPLES_PER_KERNEL) */
    uint32_t spp_offset;        /* first global sample index (progressive / sharded spp) */
    uint32_t spp_chunk;         /* samples summed per partial, 0 = spp (summation order) */
    int32_t max_depth;          /* scatter events, reference literal 7 (CUTracer.cu:212) */
    float illum;                /* emitter scale, ILLUM 10 (CV/stdafx.h:45) */
    float fov_deg;              /* horizontal FOV, 60 (CUTracer.cu:189) */
    float eye[3], dir[3], up[3];/* camera lookAt (CUTracer.cu:349-355) */
    uint64_t seed;              /* RNG seed (DESIGN.md determinism spec) */
    uint32_t prev_count;        /* running mean: fb = (fb*prev + mean)/(prev+1) (CUTracer.cu:215-217) */
    int32_t fresnel_kd;         /* 1: Fresnel multiplies Kd (CUTracer.cu:131-133); 0: not (rtx.hlsl:345) */
    int32_t tile;               /* pixel tile edge for sharding/ordering, 0 = 8 */
    int32_t shard_count;        /* tiles t with t % shard_count == shard_index are rendered; 0/1 = all */
    int32_t shard_index;
    int32_t packed;             /* 1: write owned tiles packed (tile-major) instead of row-major */
    int32_t pipeline;           /* MCPT_PIPELINE_*: megakernel (default) or wavefront; same image */
    uint32_t wf_batch;          /* wavefront: max paths per batch and stream (120 B of device memory
                                   each), 0 = automatic: LDS scenes 2^28 on one or two streams,
                                   2^27 on three or more; global-memory scenes 2^28 on one stream,
                                   2^27 on more; a default batch is also capped at work / streams
                                   and shrunk (halved) until the queues fit wf_mem_limit; where it
                                   cuts the frame of a render that can use the primary lists
                                   (mcpt_scene_primary_tile_classes) it holds whole 8x8 tiles */
    int32_t mode;               /* MCPT_MODE_*: path semantics (default CVMCTracer)       */
    int32_t lean;               /* 1: the megakernel counts only rays (paths, shades, spills,
                                   inner/leaf visits, leaf refs, triangle tests read 0; image and
                                   rays identical; ~1-2% faster); the wavefront's extend drops
                                   its traversal counters (spills, visits, refs, tests read 0;
                                   rays, paths and shades stay).  The counts are deterministic:
                                   a counting render of the same params reports what a lean one
                                   did.  0 (default): count everything */
    int32_t wf_sort;            /* wavefront: 1 = material sort (shade sorts each block of its
                                   queue by material in LDS, so a wave runs one material
                                   branch); 0 (default) = shade in queue order (dense reads,
                                   faster); same image */
    /* Scheduling.  None of these changes the image or the counters, only the
     * time; 0 = automatic (the measured defaults).
     * mcpt_plan_query reports the values a render would use.  Pinned on the
     * device, with wf_batch, against the CPU oracle: tests/test_gpu_schedules.py. */
    int32_t wf_streams;         /* wavefront HIP streams 1..4 the batches rotate over; 0: scenes in
                                   LDS 2 (3 for frames of more than 2^29 paths), global-memory scenes 4 */
    int32_t wf_refill;          /* wavefront extend: ready lanes before a wave refills (1..64);
                                   0: 16 (LDS scenes), 8 (global-memory scenes) */
    int32_t wf_group_shift;     /* wavefront, global-memory scenes: paths are dealt to queue
                                   segments in groups of 2^k (6..14); 0: 12 */
    int32_t ready_thresh;       /* megakernel: ready lanes before a shading round (1..64);
                                   0: 32 (LDS scenes), 40 (global-memory scenes) */
    int32_t tail_units_per_lane;/* megakernel tail split: the last units per lane handed out one
                                   sample at a time; 0: 4; < 0: no tail split */
    int32_t tail_units;         /* megakernel: exact number of tail-split units (overrides
                                   tail_units_per_lane when > 0) */
    uint64_t wf_mem_limit;      /* wavefront queue memory per render, bytes; 0: 90% of the device's
                                   free memory (plus what this scene already holds).  A default
                                   batch shrinks to fit; an explicit wf_batch that does not fit
                                   fails with MCPT_E_NOMEM */
    int32_t force_peer_copy;    /* multi-device renders: gather every shard with hipMemcpyPeerAsync,
                                   also between replicas on one device (exercises the cross-device
                                   path on a one-GPU box); 0: peer copies between devices only */
    int32_t gather;             /* multi-device renders (mcpt_init with a device list): how the shards
                                   reach devices[0].  MCPT_GATHER_PEER (0): one hipMemcpyPeerAsync
                                   per device (xGMI DMA).  MCPT_GATHER_RCCL: one ncclGather over a
                                   communicator of the device list (ncclCommInitAll, created on
                                   first use; librccl is loaded then) -- also for a one-device
                                   list, where it is a one-rank gather.  Same image either way */
} mcpt_render_params;

enum {
    MCPT_GATHER_PEER = 0,
    MCPT_GATHER_RCCL = 1
};

enum {
    /* CVMCTracer/CUDA/CUTracer.cu:98-218: 7 scatters + terminal query, ILLUM,
       +-1 px jitter, linear running mean, horizontal fov_deg */
    MCPT_MODE_CVMCTRACER = 0,
    /* MCRT/QuinEngine/Shader/rtx.hlsl:304-405: Russian roulette from bounce
       max_depth, stop at 3*max_depth, no ILLUM, no Fresnel Kd, +-0.5 px jitter,
       near-plane origin, gamma-2.2 running mean, t_best 10000, vertical
       fov_deg, seed = the 32-bit frame seed (GraphicsRTX.cpp:163-193) */
    MCPT_MODE_QUINENGINE = 1
};

enum {
    MCPT_PIPELINE_MEGAKERNEL = 0,   /* one persistent kernel per render (render.hip) */
    MCPT_PIPELINE_WAVEFRONT = 1     /* generate / extend / shade / accumulate queues (wavefront.hip) */
};

typedef struct {
    uint64_t rays;              /* closest-hit queries */
    uint64_t paths;
    uint64_t inner_visits;      /* inner KD nodes visited */
    uint64_t leaf_visits;
    uint64_t leaf_refs;         /* leaf triangle index reads */
    uint64_t tri_tests;
    uint64_t shades;            /* non-terminal hits shaded */
    uint64_t stack_spills;      /* traversal stack entries spilled to global memory */
    uint64_t renders;           /* render calls covered by this record */
    double kernel_ms;           /* summed GPU time of the path kernel */
    double reduce_ms;           /* summed GPU time of the partial-sum reduction */
    int32_t variant;            /* variant of the last call: megakernel 1,2 scene in LDS, 3 global;
                                   wavefront 4 scene in LDS, 5 global */
    int32_t devices;            /* devices the record covers: counters are summed over them,
                                   kernel_ms / reduce_ms are the slowest device's */
} mcpt_render_stats;

/* What a render with given params would run (mcpt_plan_query): the automatic
 * scheduling choices resolved, and the device memory it needs. */
typedef struct {
    int32_t pipeline;           /* MCPT_PIPELINE_* */
    int32_t variant;            /* kernel variant (as mcpt_render_stats::variant) */
    int32_t wf_streams;         /* wavefront streams */
    uint32_t wf_batch;          /* wavefront paths per batch and stream */
    int32_t wf_refill;
    int32_t wf_group_shift;     /* 6 for scenes in LDS (one 8x8 tile per group) */
    int32_t ready_thresh;       /* megakernel */
    int32_t tail_units;         /* megakernel tail-split units */
    uint64_t work_paths;        /* paths of the render (this device's shard) */
    uint64_t workspace_bytes;   /* device memory the render's workspace needs */
    uint64_t wf_queue_bytes;    /* of which the wavefront's queues (what wf_mem_limit bounds) */
    uint64_t device_free_bytes; /* free memory of the scene's device now */
    int32_t devices;            /* devices the render runs on */
    int32_t peer_access;        /* multi-device: 1 if peer access between every pair is enabled */
    uint32_t wf_batch_default;  /* wavefront: the batch the schedule picks with memory unbounded;
                                   wf_batch below it = the queues were shrunk to fit (wf_mem_limit,
                                   the scene's reservation or free device memory) -- ABI 8 */
} mcpt_plan_info;

/* Scene creation options (mcpt_scene_create_ex). */
typedef struct {
    const char* kd_cache_dir;   /* on-disk KD-build cache directory (must exist); NULL = none */
    int32_t host_only;          /* 1: no device allocation */
    int32_t layout;             /* MCPT_LAYOUT_*: scene image placement */
    int32_t kd_build;           /* MCPT_KD_BUILD_*: the KD tree's split rule -- ABI 9 */
} mcpt_scene_options;

enum {
    MCPT_LAYOUT_AUTO = 0,       /* LDS image (8-B nodes) when it fits, else global memory with child boxes */
    MCPT_LAYOUT_GLOBAL = 1      /* global memory with 48-B child-box pair records, whatever the size */
};
/* KD split rule.  Images do not depend on it (the closest hit is the
 * brute-force one for any tree); visit counts and speed do. */
enum {
    MCPT_KD_BUILD_REFERENCE = 0,  /* QuinEngine KDTree.hpp:58-287: median > 64 tris, SAH with Cts = 0 below */
    MCPT_KD_BUILD_SAH = 1         /* SAH with a traversal cost over split-plane regions at every size
                                     (empty space cut off): fewer node visits per ray (host_model.cpp) */
};

/* ---- library ------------------------------------------------------------ */
int mcpt_abi_version(void);
const char* mcpt_last_error(void);
/* Initialize (CUTracer.cu:220-223): select the HIP device(s) used by later
 * scene_create calls on this thread; devices[0] becomes current and holds the
 * scene.  n_devices > 1: the scene is replicated on every listed device, and
 * each unsharded render (shard_count <= 1, packed = 0) is split into
 * n_devices interleaved-tile shards (tile t -> device t % n), rendered
 * concurrently, peer-copied to devices[0] (xGMI DMA) and unpermuted there --
 * the single-device image bit for bit; stats sum the devices.  A device may
 * be listed twice (two replicas on one GPU; RCCL refuses such a list for its
 * gather, mcpt_render_params::gather).  n_devices == 0 keeps the current
 * device and a single-device scene. */
int mcpt_init(const int32_t* devices, int32_t n_devices);
int mcpt_device_count(int32_t* out);
/* fill defaults = the CVMCTracer constants for scene 1 (CUTracer.cu:347-360) */
void mcpt_render_params_default(mcpt_render_params* p);
/* QuinEngine viewer defaults (GraphicsRTX.cpp:163-193, rtx.hlsl:373-404):
 * mode QE, 640x480 (the QE window, QE/Main.cpp:11), 1 spp per frame, depth 5,
 * fovY 45, eye (0,5,17)                                                       */
void mcpt_render_params_quinengine(mcpt_render_params* p);

/* ---- host model (ObjModel) ---------------------------------------------- */
/* In-memory ObjModel, laid out like ObjReader.hpp:57-63 (element 0 of every
 * array is the reference's dummy).  Groups in CSR form, any order (they are
 * re-keyed by name like the reference's std::map).  Arrays are copied.     */
typedef struct {
    const float* vertices;        int64_t n_vertices;    /* 3 floats each  */
    const float* normals;         int64_t n_normals;     /* 3 floats each  */
    const int32_t* triangles;     int64_t n_triangles;   /* 10 ints each: v[3] t[3] n[3] material */
    const double* materials;      int64_t n_materials;   /* 12 doubles each: Ka Kd Ks Ns Tr Ni */
    const char* const* group_names;                      /* n_groups names */
    const int64_t* group_offsets;                        /* n_groups+1 offsets into group_tris */
    const int32_t* group_tris;    int64_t n_groups;
} mcpt_model_desc;
int mcpt_model_create(const mcpt_model_desc* d, mcpt_model** out);
int mcpt_model_read_obj(const char* path, mcpt_model** out);
/* The same with a reader flavor: MCPT_OBJ_CVMCTRACER = mcpt_model_read_obj;
 * MCPT_OBJ_TINYOBJ = what QuinEngine loads through tinyobjloader v1.1.1
 * (QE/Utils/Structure.hpp:9-12, RTX/ShaderResource.hpp:88-104, 204-215):
 * materials with tinyobj's defaults (Ka Kd Ks 0, Ns 1, Ni 1; Tr = 1 - dissolve,
 * `d` wins over `Tr`), shapes in file order, a material per triangle (a group
 * per run of one shape's faces with one material, keyed "%06d:<shape>"). */
int mcpt_model_read_obj_ex(const char* path, int32_t flavor, mcpt_model** out);
enum {
    MCPT_OBJ_CVMCTRACER = 0,    /* CVMCTracer ObjReader (ObjReader.cpp:8-259) */
    MCPT_OBJ_TINYOBJ = 1        /* QuinEngine's tinyobjloader */
};
void mcpt_model_free(mcpt_model* m);
int mcpt_model_get_info(const mcpt_model* m, mcpt_model_info* out);
int mcpt_model_copy_vertices(const mcpt_model* m, float* out);       /* n_vertices*3 */
int mcpt_model_copy_normals(const mcpt_model* m, float* out);        /* n_normals*3 */
int mcpt_model_copy_triangles(const mcpt_model* m, int32_t* out);    /* n_triangles*10: v[3] t[3] n[3] mat */
int mcpt_model_copy_materials(const mcpt_model* m, double* out);     /* n_materials*12: Ka Kd Ks Ns Tr Ni */
/* group g (std::map order): name into buf, triangle count in *n; copy indices if tris != NULL */
int mcpt_model_group(const mcpt_model* m, int64_t g, char* name_buf, int64_t name_cap,
                     int64_t* n, int32_t* tris);

/* ---- scene (CreateGeometry / DestroyGeometry) ---------------------------- */
/* Builds geometries, the KD tree and the device image on the current device.
 * The model is borrowed for the duration of the call only.                 */
int mcpt_scene_create(const mcpt_model* m, mcpt_scene** out);
/* Same, but host-only: no device allocation (KD inspection / CPU tests).   */
int mcpt_scene_create_host(const mcpt_model* m, mcpt_scene** out);
/* Same as mcpt_scene_create (host_only = 0) / _create_host (host_only = 1),
 * with an on-disk KD-build cache in kd_cache_dir (must exist; NULL or "" =
 * no cache).  The tree is a pure function of the triangle vertices, keyed by
 * two 64-bit hashes of them; a file that fails any check is rebuilt and
 * rewritten.  *cache_hit (may be NULL) = 1 if the tree was read, 0 if built.
 * (the reference rebuilds its tree on every start,
 * QuinEngine/RTX/ShaderResource.hpp:128-179.)                              */
int mcpt_scene_create_cached(const mcpt_model* m, const char* kd_cache_dir, int32_t host_only,
                             mcpt_scene** out, int32_t* cache_hit);
/* General form of the three above (options may be NULL = defaults). */
int mcpt_scene_create_ex(const mcpt_model* m, const mcpt_scene_options* options, mcpt_scene** out,
                         int32_t* cache_hit);
void mcpt_scene_destroy(mcpt_scene* s);
int mcpt_scene_get_info(const mcpt_scene* s, mcpt_scene_info* out);
/* Emitter boxes of the wavefront's terminal cull (1..8: one per emitter
 * geometry), or 0 when the scene does not allow it: a non-emitter with a Ka
 * other than zero, a non-finite Kd or Ks, no emitter, or more than 8.  (Its own
 * entry: mcpt_scene_info keeps its ABI 9 size.) */
int mcpt_scene_terminal_cull_boxes(const mcpt_scene* s);
/* Occluder boxes of the wavefront's miss cull (1..8 fp32 AABBs that together
 * hold every triangle; lean renders end a path whose new ray misses them all),
 * or 0 when the scene has none: a box would span the scene bounds, or the
 * scene is a closed room.  boxes (may be NULL): 6 floats per box, min xyz then
 * max xyz.  (Its own entry, as the one above; an addition, the ABI stays 9.) */
int mcpt_scene_miss_cull_boxes(const mcpt_scene* s, float* boxes);
/* Direct lists of the wavefront (lean renders of a scene in LDS with occluder
 * boxes): every triangle is assigned to one occluder box that holds it, and a
 * box with 1..K triangles is small -- a secondary ray whose segment hits that
 * box alone is resolved from the box's triangles without a tree walk, same hit.
 * Returns K (0: built without the lists).  Each pointer may be NULL:
 * tri_box[n_triangles] = kd id -> box index (as mcpt_scene_miss_cull_boxes
 * orders them); box_tris[8] = triangles assigned to each box; lists[8 * K] =
 * per small box its triangles' record indices (3 x the image triangle slot:
 * the hit ids' and leaf references' unit) in image order, zeros for the other
 * boxes; list_kd[8 * K] = the same entries as kd ids, -1 where a list has
 * none.  (Its own entry, as the ones above; an addition, the ABI stays 9.) */
int mcpt_scene_direct_lists(const mcpt_scene* s, int32_t* tri_box, uint32_t* box_tris, uint32_t* lists,
                            int32_t* list_kd);
/* The direct rays of the stats record last read from the scene (mcpt_render's,
 * mcpt_render_stats_read's): secondary rays the shades marked for their box's
 * list, summed over devices.  0 wherever the lists are off: counting renders,
 * the megakernel, a scene in global memory or without boxes.  They are counted
 * in mcpt_render_stats::rays like every other ray. */
uint64_t mcpt_scene_direct_rays(const mcpt_scene* s);
/* The rays the wavefront's secondary extends (bounce >= 1) took, of the same
 * stats record, summed over devices: every secondary ray but the direct ones
 * (the shade that makes them resolves them) and those the miss cull and the
 * terminal cull answer.  0 for the megakernel and in a build without the direct
 * resolve.  (An addition, as the one above; the ABI stays 9.) */
uint64_t mcpt_scene_extend_rays(const mcpt_scene* s);
/* Of those, the rays an extend started with a selector (the clip walk: a ray
 * through at least one box without a list and at most one with a list walks
 * only inside its unlisted boxes' slab interval, its listed box's triangles
 * tested first).  0 wherever the direct lists are off, and in a build without
 * the clip walk.  (An addition, as the ones above; the ABI stays 9.) */
uint64_t mcpt_scene_clipped_rays(const mcpt_scene* s);
/* Paths of the stats record last read whose bounce 0 was shaded by the kernel
 * that resolved their primary rays (wavefront, lean CV renders of a scene in
 * LDS with occluder boxes, 8x8 tiles, batches of whole tiles, wf_sort 0): equal
 * to the record's paths there, 0 for every other render.  (An addition, as the
 * ones above; the ABI stays 9.) */
uint64_t mcpt_scene_primary_shaded(const mcpt_scene* s);
/* Sphere clip: the occluder boxes without a list that have a sphere over their
 * triangles' vertices which cuts something off the box -- bit i of the result:
 * box i of mcpt_scene_miss_cull_boxes; spheres (NULL, or room for 8 x 4 floats)
 * receives {centre xyz, radius^2} per box, zeros for a box without one.  A lean
 * wavefront render of a scene in LDS whose clip walk is active cuts a clipped
 * ray's walk to its boxes' spheres.  (An addition; the ABI stays 9.) */
uint32_t mcpt_scene_clip_spheres(const mcpt_scene* s, float* spheres);
/* Of the clipped rays of the stats record last read, those whose walk was not
 * started because a sphere left nothing of their interval; 0 for every render
 * that does not clip to spheres.  (An addition; the ABI stays 9.) */
uint64_t mcpt_scene_sphere_skips(const mcpt_scene* s);
/* LDS bytes per workgroup that such a render's bounce-0 kernel is launched
 * with (all of it dynamic: the kernel has no static LDS), from the same
 * function the launch calls; 0 for a scene that is not rendered from LDS.
 * (An addition; the ABI stays 9.) */
uint64_t mcpt_scene_primary_shade_lds(const mcpt_scene* s);
/* Primary lists of the scene's last render (wavefront, lean CV renders of a
 * scene in LDS with 8x8 tiles): out[0..2] = the owned tiles whose candidate
 * list is empty (no primary ray made), holds 1..K triangles (tested straight
 * from the list) or more than K (the packet walk), out[3] = K (0: built
 * without the lists).  All three are 0 after a render that did not use the
 * lists.  A batch reads the lists only if its pixel range is whole tiles; the
 * batch split is known on the host before anything is launched, so a render
 * none of whose batches is whole tiles (wf_batch = 1000 on a frame of more
 * pixels, say) runs no candidate pass and reports 0 0 0, and a render with at
 * least one such batch runs the pass once and reports every owned tile, also
 * those whose batches walked.  tests/test_gpu_schedules.py pins both.  Waits
 * for the device.  (Its own entry, as the one above.) */
int mcpt_scene_primary_tile_classes(mcpt_scene* s, uint32_t out[4]);
/* KD tree as built (BFS order, QuinEngine/RTX/ShaderResource.hpp:128-179):
 * nodes n_nodes*12 words {left,right,axis(0 leaf,1..3),split bits,min[3],max[3],
 * leaf_begin,leaf_count}; leaf ids = kd triangle ids; kd_tris = kd id -> OBJ
 * triangle index; geoms n_geometries*14 floats {Ka Kd Ks Ns Tr Ni start count} */
int mcpt_scene_copy_kd(const mcpt_scene* s, uint32_t* nodes, uint32_t* leaf_ids,
                       int32_t* kd_tris, float* geoms);

/* ---- render (RenderScene) ------------------------------------------------- */
/* Synchronous; fb_rgb is caller-owned host memory, width*height*3 floats
 * (or, when packed/sharded, owned-pixel-count*3).  Reads fb_rgb when
 * prev_count > 0.  stats may be NULL.                                        */
int mcpt_render(mcpt_scene* s, const mcpt_render_params* p, float* fb_rgb, mcpt_render_stats* stats);
/* Asynchronous on hip_stream (a hipStream_t, NULL = default stream);
 * d_fb_rgba is device memory, 4 floats per output pixel.  Counters and
 * kernel times accumulate until mcpt_render_stats_read(), which waits for
 * the outstanding calls and resets them.                                   */
int mcpt_render_device(mcpt_scene* s, const mcpt_render_params* p, float* d_fb_rgba, void* hip_stream);
int mcpt_render_stats_read(mcpt_scene* s, mcpt_render_stats* out);
/* Diagnostics: synchronous render that also returns, per work unit
 * u = chunk*pixels + pixel, {rays, inner visits, leaf visits, tri tests}
 * (unit_counters: total_units*4 uint32, total_units = pixels * ceil(spp/chunk)). */
int mcpt_render_unit_counters(mcpt_scene* s, const mcpt_render_params* p, float* fb_rgb,
                              uint32_t* unit_counters);
/* number of output pixels a (sharded) render writes, and their (x,y) list */
int64_t mcpt_shard_pixel_count(const mcpt_render_params* p);
int mcpt_shard_pixels(const mcpt_render_params* p, int32_t* xy);      /* count*2 */
/* Closest hit of n caller-given rays on the scene's device, the reference's
 * intersect() (CUTracer.cu:44-96) through the traversal the renders use (the
 * ordered KD walk; scenes in global memory with the child-box cull):
 * o, d = n*3 floats (host); tri_out[i] = kd triangle id (scene_copy_kd's
 * numbering) or -1; hit_out = n*3 floats beta, gamma, t (t = 0 on a miss);
 * t_max = the initial closest t (FLT_MAX in CVMCTracer, 10000 in QuinEngine).
 * stats (may be NULL): rays, inner/leaf visits, leaf refs, tri tests.
 * Ray preconditions (this entry and the device queries below): finite
 * origins, anywhere -- inside the scene's box, on its faces or outside it --
 * and finite directions, not all zero, whose every component is zero (+0.0
 * or -0.0 alike) or has a finite float reciprocal; |d| >= 2^-126 (any normal
 * float) suffices.  Directions need not have unit length: t comes back in
 * units of the given direction, and scaling a direction by 2^k divides t by
 * 2^k and changes nothing else (pinned for |k| <= 40).  Inside this range the
 * answer is the brute force's of CUTracer.cu:44-96, bit for bit, except for
 * origins exactly on a triangle's edge.  Outside
 * it -- a subnormal component whose reciprocal overflows -- the entries
 * return the ordered walk's answer, which is defined and the same on every
 * layout but can miss a hit the brute force finds at t near FLT_MAX; NaN and
 * infinite rays are not supported.  (tests/test_ray_contract_cpu.py,
 * tests/test_gpu_ray_contract.py)                                          */
int mcpt_intersect(mcpt_scene* s, int64_t n, const float* o, const float* d, float t_max,
                   int32_t* tri_out, float* hit_out, mcpt_render_stats* stats);
/* reserve device workspace for p so mcpt_render_device allocates nothing
 * (required before hipGraph capture).  Megakernel workspace per render:
 * partial sums 16 B x pixels x ceil(spp/chunk), the tail-split buffer (16 B
 * per sample of the last ~4 units per lane) and the stack spill area (32 x
 * 16 B per lane); wavefront: 120 B per path of the batch.
 * After a reserve, a render on a CAPTURING stream that needs more than the
 * scene holds fails with MCPT_E_NOMEM before any launch; a render on a
 * non-capturing stream grows the workspace, and the buffers it outgrows are
 * kept (not freed) until mcpt_scene_destroy, so a graph captured earlier
 * stays valid.                                                               */
int mcpt_scene_reserve(mcpt_scene* s, const mcpt_render_params* p);
/* The scheduling a render of p would use and its memory (no allocation, no
 * launch), for a render on a stream that is not capturing a graph (a
 * captured render is held to the scene's reservation, mcpt_scene_reserve).  */
int mcpt_plan_query(mcpt_scene* s, const mcpt_render_params* p, mcpt_plan_info* out);

/* ---- first-hit feature buffers (AOVs) and the denoiser --------------------- */
/* Per-pixel features of the render's own primary rays: for the samples
 * spp_offset .. spp_offset + spp - 1 of p, the ray the render of p traces
 * first (same RNG stream, jitter and camera) and its closest hit through the
 * renders' traversal.  Two row-major buffers, 4 floats per pixel, each channel
 * the plain fp32 mean over the samples (a miss counts as zeros):
 *   albedo_cov   = r g b coverage: the factor the first scatter multiplies into
 *                  the throughput -- (1,1,1) on an emitter; Tr > 0: Kd if
 *                  fresnel_kd (CVMCTracer mode only) else (1,1,1); Ns > 1: Ks;
 *                  else Kd -- and 1 for a hit
 *   normal_depth = nx ny nz t: the shading normal as the scatter forms it
 *                  (interpolated, normalized, not flipped) and the hit's t
 * prev_count > 0: each channel becomes (old * prev_count + mean) / (prev_count + 1),
 * the linear running mean in both modes (the buffers are read).
 * The call takes its own spp -- features converge with far fewer samples than
 * radiance (1 to 16 is plenty) -- and ignores spp_chunk, max_depth, pipeline
 * and the scheduling fields.  shard_count > 1 or packed: MCPT_E_UNSUPPORTED.
 * A multi-device scene computes them on devices[0].  The scene's render stats
 * are not touched.  The workspace is the scene's (the stack spill area a
 * render of the same scene uses): after mcpt_scene_reserve(p) or a first call
 * nothing is allocated.  Run it on the stream of the scene's renders, or
 * synchronize: they share that workspace.                                   */
int mcpt_render_aov(mcpt_scene* s, const mcpt_render_params* p, float* albedo_cov, float* normal_depth);
/* The same on device buffers (4 floats per pixel each), asynchronous on hip_stream. */
int mcpt_render_aov_device(mcpt_scene* s, const mcpt_render_params* p, float* d_albedo_cov, float* d_normal_depth,
                           void* hip_stream);

/* Edge-avoiding a-trous denoiser (Dammertz et al., HPG 2010) on
 * albedo-demodulated colour, guided by the two feature buffers; fp32, a fixed
 * operation order.  0 in a field = its default. */
typedef struct {
    int32_t width, height;
    int32_t iterations;         /* a-trous passes, step 2^i; 0 = 5, at most 8 */
    int32_t normal_power_log2;  /* normal weight = clamp(n.n', 0, 1)^(2^k); 0 = 7 (power 128), at most 10 */
    float sigma_z;              /* relative depth tolerance; 0 = 0.1 */
    float albedo_floor;         /* demodulation divides by max(albedo, floor); 0 = 0.01 */
    int32_t gamma_space;        /* 1: colour is gamma-2.2 encoded (a QuinEngine-mode framebuffer):
                                   decoded before, encoded after */
} mcpt_denoise_params;
/* the defaults spelled out (5, 7, 0.1, 0.01, linear colour); width and height 0 */
void mcpt_denoise_params_default(mcpt_denoise_params* p);
/* Host buffers, synchronous, on the current device: colour in and out 3 floats
 * per pixel, features 4.  out_rgb may not overlap an input.                   */
int mcpt_denoise(const mcpt_denoise_params* p, const float* color_rgb, const float* albedo_cov,
                 const float* normal_depth, float* out_rgb);
/* Device buffers of 4 floats per pixel, asynchronous on hip_stream, no
 * allocation: d_color_rgba is only read (alpha ignored), d_out_rgba receives
 * the result (alpha 0), d_scratch_rgba is a work buffer of the same size;
 * neither may overlap another buffer of the call.                           */
int mcpt_denoise_device(const mcpt_denoise_params* p, const float* d_color_rgba, const float* d_albedo_cov,
                        const float* d_normal_depth, float* d_out_rgba, float* d_scratch_rgba, void* hip_stream);

/* ---- per-pixel variance and the variance-guided denoiser ------------------- */
/* mcpt_render plus the variance of this call's pixel mean: the render of p
 * (framebuffer, stats and counters bit-identical to mcpt_render's) followed by
 * one kernel on the same stream that reads the per-chunk partial sums the
 * render wrote.  var_rgba is row-major, 4 floats per pixel (var_r var_g var_b 0),
 * linear radiance squared in both modes (the QuinEngine gamma applies to the
 * framebuffer only).  A batch-means estimate over the K = ceil(spp / spp_chunk)
 * chunks, fp32 in a fixed operation order:
 *   mean = (P_0 + ... + P_K-1) / spp          P_c: chunk c's sum, n_c samples
 *   var  = sum_c n_c (P_c / n_c - mean)^2 / (spp (K - 1))
 * prev_count > 0: var = (old prev_count^2 + var) / (prev_count + 1)^2, the
 * variance of the render's equal-weight running mean (the buffer is read).
 * K < 2 (spp_chunk = 0 is one chunk): MCPT_E_INVALID.  shard_count > 1,
 * packed, a multi-device scene or gather = RCCL: MCPT_E_UNSUPPORTED.  The
 * variance step allocates nothing: after mcpt_scene_reserve(p) neither does
 * mcpt_render_var_device.                                                   */
int mcpt_render_var(mcpt_scene* s, const mcpt_render_params* p, float* fb_rgb, float* var_rgba,
                    mcpt_render_stats* stats);
/* The same on device buffers (4 floats per pixel each, not overlapping),
 * asynchronous on hip_stream as mcpt_render_device.                          */
int mcpt_render_var_device(mcpt_scene* s, const mcpt_render_params* p, float* d_fb_rgba, float* d_var_rgba,
                           void* hip_stream);

/* mcpt_denoise with an SVGF-style luminance edge-stopping weight (Schied et
 * al., HPG 2017) driven by that variance, which is filtered along with the
 * colour: a tap's weight is also multiplied by max(1 - |l_p - l_q| /
 * (sigma_l sqrt(g_p) + 1e-6), 0)^2, l the luminance of the demodulated colour
 * and g_p the 3x3-prefiltered luminance variance.     */
typedef struct {
    mcpt_denoise_params base;
    float sigma_l;              /* luminance tolerance in standard deviations; 0 = 4 */
} mcpt_denoise_var_params;
/* mcpt_denoise_params_default for base, sigma_l 4 */
void mcpt_denoise_var_params_default(mcpt_denoise_var_params* p);
/* Buffers, overlap rules and checks as mcpt_denoise; var_rgba (4 floats per
 * pixel, of mcpt_render_var, always linear) is one more read-only input.    */
int mcpt_denoise_var(const mcpt_denoise_var_params* p, const float* color_rgb, const float* var_rgba,
                     const float* albedo_cov, const float* normal_depth, float* out_rgb);
/* As mcpt_denoise_device, with d_var_rgba one more read-only input.         */
int mcpt_denoise_var_device(const mcpt_denoise_var_params* p, const float* d_color_rgba, const float* d_var_rgba,
                            const float* d_albedo_cov, const float* d_normal_depth, float* d_out_rgba,
                            float* d_scratch_rgba, void* hip_stream);

/* ---- temporal accumulation --------------------------------------------------- */
/* The temporal half of that filter, between "render" and "denoise": a frame's
 * history reprojected onto a new camera.  (Additions; the ABI stays 9.)  For
 * every pixel of the new frame (camera cur) the surface point its features
 * give -- the pixel centre's ray at the mean hit distance normal_depth.w /
 * coverage -- is projected into the previous frame (camera prev); the
 * accumulated colour, history length N and variance are fetched there
 * bilinearly from the taps that show the same surface (the previous frame's
 * features: coverage > 0, normals and depth within the two tolerances below),
 * from the valid pixels of the 3x3 block around the nearest pixel if no
 * bilinear tap is one, and blended with this frame:
 *   Ne = min(N, max_history - 1)
 *   out     = ((hist Ne + colour) / (Ne + 1), Ne + 1)
 *   out_var = ((hist_var Ne Ne + var) / (Ne + 1)^2, 0)
 * the renders' running mean and mcpt_render_var's merge.  A pixel that hit
 * nothing, whose point lies behind or outside the previous frame or finds no
 * valid tap is reset: out = (colour, 1), out_var = (var, 0); out.w == 1 marks
 * it.  fp32 in a fixed operation order.  Static
 * geometry only; the caller ping-pongs: this call's outputs and this frame's
 * feature buffers are the next call's history.  0 in a field = its default.   */
typedef struct {
    int32_t max_history;      /* cap on a pixel's history length; 0 = 32; 1..65536.  1 = no accumulation */
    float   normal_threshold; /* a tap is the same surface if dot(n_p, n_q) >= thr * (cov_p * cov_q); 0 = 0.9; (0, 1] */
    float   sigma_z;          /* ... and |e - z_q| <= sigma_z * max(e, z_q), e the depth expected there;
                                 0 = 0.1 (mcpt_denoise's default); > 0, finite */
    int32_t gamma_space;      /* 1: d_color is gamma-2.2 encoded (a QuinEngine-mode framebuffer): decoded on read.
                                 History and outputs are always linear */
} mcpt_temporal_params;
/* the defaults spelled out: 32, 0.9, 0.1, 0 */
void mcpt_temporal_params_default(mcpt_temporal_params*);
/* Device buffers, row-major, 4 floats per pixel, asynchronous on hip_stream, no
 * allocation (capturable in a graph, as mcpt_denoise_device).  This frame:
 * d_color_rgba (alpha ignored), d_var_rgba (of mcpt_render_var), d_albedo_cov
 * and d_normal_depth (of mcpt_render_aov).  History: d_hist_color_n (r g b N),
 * d_hist_var and the previous frame's two feature buffers.  d_var_rgba,
 * d_hist_var and d_out_var are given together or all NULL (no variance is
 * carried); tp may be NULL (the defaults).  Of cur and prev only width,
 * height, fov_deg, eye, dir, up and mode are read; width, height and mode must
 * be equal in both.  Checks, before any launch and in this order:
 * MCPT_E_INVALID for a NULL required pointer, a field of tp out of range (the
 * message names it), width or height <= 0, an unknown mode, cur and prev
 * mismatched (the message names the field), the variance pointers given
 * partially; MCPT_E_UNSUPPORTED for width x height >= 2^31 / 3; MCPT_E_INVALID
 * for an output that overlaps an input or the other output.                  */
int mcpt_temporal_device(const mcpt_temporal_params* tp, const mcpt_render_params* cur, const mcpt_render_params* prev,
                         const float* d_color_rgba, const float* d_var_rgba, const float* d_albedo_cov,
                         const float* d_normal_depth, const float* d_hist_color_n, const float* d_hist_var,
                         const float* d_hist_albedo_cov, const float* d_hist_normal_depth, float* d_out_color_n,
                         float* d_out_var, void* hip_stream);
/* The same on host arrays, synchronous, on the current device; colour in and
 * out 4 floats per pixel here too (the alpha of hist_color_n and out_color_n
 * carries N).  Every check comes before anything is staged.                   */
int mcpt_temporal(const mcpt_temporal_params* tp, const mcpt_render_params* cur, const mcpt_render_params* prev,
                  const float* color_rgba, const float* var_rgba, const float* albedo_cov, const float* normal_depth,
                  const float* hist_color_n, const float* hist_var, const float* hist_albedo_cov,
                  const float* hist_normal_depth, float* out_color_n, float* out_var);

/* ---- variance-driven adaptive sampling -------------------------------------- */
/* Passes of p->spp samples, each pass only over the pixels that are still
 * noisy.  Pass 0 is mcpt_render_var of p for every pixel.  Before pass j >= 1
 * every pixel gets, from the current framebuffer and variance (fp32, one
 * rounding per operation; k = (0.2126, 0.7152, 0.0722)),
 *   sd_c = sqrt(max(var_c, 0))
 *   s    = (k.x sd_r + k.y sd_g) + k.z sd_b
 *   l    = (k.x fb_r + k.y fb_g) + k.z fb_b
 *   over = s > threshold (l + lum_floor)
 * and pass j renders the pixels that were active in pass j - 1 and have an
 * `over` pixel in their (2r+1)^2 window (clipped to the image); for
 * j < min_passes, and as the predecessor of pass min_passes, every pixel is
 * active.  A pixel that stopped never restarts; an empty set ends the render.
 * The active pixels are rendered as a uniform mcpt_render_var with
 * spp_offset + j spp and prev_count = j renders them (same chunks, partial
 * sums, running mean and variance merge), so a pixel with pass_count m holds,
 * bit for bit, what m chained uniform mcpt_render_var calls leave in it, and
 * the counters are the sums over the pixels rendered.
 * The pixel list is built on the device (selection, per-block ballot counts,
 * scan, scatter in tile-major order); the host reads its length once per pass. */
typedef struct {
    int32_t max_passes;   /* passes of p->spp samples a pixel can get; 0 = 8; 1..4096 */
    int32_t min_passes;   /* passes every pixel gets before selection starts; 0 = 1; <= max_passes */
    float   threshold;    /* stop a pixel when the standard error of its luminance <= threshold * (luminance + lum_floor); 0 = 0.2; >= 0 */
    float   lum_floor;    /* 0 = 0.01; >= 0 */
    int32_t dilate;       /* radius r of the (2r+1)^2 window over which "still noisy" spreads; 0 = 1; < 0 = none; at most 4 */
    int32_t force_list;   /* 1: full-frame passes after pass 0 also run through the pixel list (measures the list's overhead; same result) */
} mcpt_adaptive_params;
/* max_passes 8, min_passes 1, threshold 0.2, lum_floor 0.01, dilate 1, force_list 0 */
void mcpt_adaptive_params_default(mcpt_adaptive_params*);
/* fb_rgb: 3 floats per pixel; var_rgba: 4; pass_count: one uint32 per pixel
 * (all row-major, written only).  stats: counters summed over the passes,
 * renders = passes run.  a may be NULL (the defaults).  MCPT_E_INVALID:
 * whatever mcpt_render_var rejects, prev_count != 0, spp_offset +
 * max_passes * spp past 2^32, an adaptive field out of range.
 * MCPT_E_UNSUPPORTED: whatever mcpt_render_var refuses, the wavefront
 * pipeline, QuinEngine mode, a capturing stream (the host reads the list's
 * length each pass).  All checks come before any launch.                     */
int mcpt_render_adaptive(mcpt_scene*, const mcpt_render_params*, const mcpt_adaptive_params*,
                         float* fb_rgb, float* var_rgba, uint32_t* pass_count, mcpt_render_stats* stats);
/* The same on device buffers (4 floats per pixel for d_fb_rgba and d_var_rgba,
 * none overlapping).  The call waits for hip_stream once per selecting pass;
 * the last pass is left running on it.  After mcpt_scene_reserve(p) and one
 * call a further call allocates nothing.                                      */
int mcpt_render_adaptive_device(mcpt_scene*, const mcpt_render_params*, const mcpt_adaptive_params*,
                                float* d_fb_rgba, float* d_var_rgba, uint32_t* d_pass_count, void* hip_stream);
/* The general form: the pair above with p->pipeline honoured.  (The pair above
 * is the megakernel-only form, kept for its callers: it refuses the wavefront
 * as it always did.  Additions; the ABI stays 9.)  Arguments, buffers,
 * semantics, checks and their order are the pair's, minus the pipeline
 * refusal.  With MCPT_PIPELINE_MEGAKERNEL the calls are the pair's, same code
 * path, bits and counters.  With MCPT_PIPELINE_WAVEFRONT pass 0 and every
 * full-frame pass before min_passes (without force_list) are the wavefront's
 * uniform mcpt_render_var renders as they are, primary lists, primary shade
 * and culls included; a listed pass of n pixels is a wavefront render of a
 * frame of n listed pixels: its generate kernel looks each pixel up in the
 * list and writes an explicit queue 0, bounce 0 runs the ordinary extend and
 * shade (no packet extend, primary lists or primary shade), and the miss
 * cull, direct lists, direct resolve, clip walk and terminal cull stay on.
 * wf_batch, wf_streams, wf_refill, wf_group_shift, wf_sort, wf_mem_limit, lean
 * and tile are honoured as by a wavefront mcpt_render_var; a listed pass runs
 * on pass 0's streams with the default batch of a frame of n pixels (an
 * explicit wf_batch as asked), never more than pass 0's, inside pass 0's
 * workspace.  fb, var and pass_count are the megakernel's bit for bit, as are
 * paths (spp x the sum of pass_count), renders and rays; a counting render's
 * (lean = 0) inner_visits, leaf_visits, leaf_refs and tri_tests too, a lean
 * one's read 0 as for every lean wavefront render.  direct_rays, extend_rays
 * and clipped_rays accumulate over the passes; primary_shaded counts the
 * eligible paths of the full-frame passes only (a listed pass adds 0).
 * mcpt_scene_primary_tile_classes reports the last pass: 0 0 0 after a render
 * whose last pass was listed, as after any render that did not use the lists.
 * Still MCPT_E_UNSUPPORTED, with the pair's messages: QuinEngine mode, a
 * capturing stream, shards, packed output, a multi-device scene, gather = RCCL. */
int mcpt_render_adaptive_ex(mcpt_scene*, const mcpt_render_params*, const mcpt_adaptive_params*,
                            float* fb_rgb, float* var_rgba, uint32_t* pass_count, mcpt_render_stats* stats);
int mcpt_render_adaptive_ex_device(mcpt_scene*, const mcpt_render_params*, const mcpt_adaptive_params*,
                                   float* d_fb_rgba, float* d_var_rgba, uint32_t* d_pass_count, void* hip_stream);

/* ---- device ray queries: closest hit and any hit over ray buffers ------------ */
/* The renders' traversal for rays of the caller's own, in device memory: a
 * query is the walk mcpt_intersect runs (the ordered KD walk with the scene's
 * layout: the LDS image, or the global-memory image with the child-box cull),
 * in a persistent kernel built like the wavefront extend.  Asynchronous on a
 * stream; after mcpt_scene_reserve_rays or a first query nothing is allocated.
 * Preconditions as mcpt_intersect ("Ray preconditions" there): finite origins,
 * inside or outside the scene's box; finite directions, not all zero, of any
 * length (t in units of the given direction), each component zero of either
 * sign or with a finite float reciprocal (|d| >= 2^-126 suffices) -- outside
 * that range the walk's answer, not the brute force's, is returned;
 * t_max finite or FLT_MAX (a t_max <= 0 simply misses).
 * MCPT_E_INVALID, before anything is launched or allocated and in this order:
 * a NULL scene, n < 0, a NULL required pointer with n > 0, a field of the
 * params out of range (the message names it); then MCPT_E_UNSUPPORTED for
 * n >= 2^31 / 3 (mcpt_intersect's limit); then MCPT_E_INVALID for a host-only
 * scene and for an output buffer that overlaps an input or another output.
 * n = 0 is a no-op.  A multi-device scene runs the query on devices[0].
 * The workspace is the scene's: the stack spill area a render of the same
 * scene uses (32 x 16 B per resident lane), a device copy of the triangle
 * numbering (4 B per triangle) and a counter block.  Run the queries on the
 * stream of the scene's renders, or synchronize: they share the spill area. */
enum { MCPT_TRACE_CLOSEST = 0, MCPT_TRACE_ANY = 1 };
typedef struct {
    int32_t kind;        /* MCPT_TRACE_* */
    float   t_max;       /* initial closest t for every ray when no per-ray array is given; 0 = FLT_MAX
                            (QuinEngine's t_best is 10000); must be >= 0 */
    int32_t lean;        /* 1: traversal counters compiled out (rays still counted) */
    int32_t workgroups;  /* scheduling only, never changes a result: 0 = automatic; > 0 = at most this many
                            persistent workgroups (1 makes one workgroup refill over the whole batch) */
    int32_t refill;      /* scheduling only: ready lanes before a wave refills, 1..64; 0 = the extend's default
                            for the scene's layout */
} mcpt_trace_params;
void mcpt_trace_params_default(mcpt_trace_params*);   /* all zeros spelled out: CLOSEST, FLT_MAX */

/* n rays; d_o, d_d: n*3 floats each (mcpt_intersect's layout); d_t_max: n floats or NULL (p->t_max for all).
 * CLOSEST: d_tri[i] = kd triangle id (mcpt_scene_copy_kd's numbering) or -1; d_hit (may be NULL): n*3 floats
 * beta, gamma, t, and (0,0,0) on a miss -- exactly what mcpt_intersect returns for the same ray and t_max.
 * Asynchronous on hip_stream.  p may be NULL (the defaults).  p->kind = MCPT_TRACE_ANY here is
 * MCPT_E_UNSUPPORTED: the any-hit query reports a flag, not a triangle (mcpt_occluded_device). */
int mcpt_trace_device(mcpt_scene*, const mcpt_trace_params* p, int64_t n, const float* d_o, const float* d_d,
                      const float* d_t_max, int32_t* d_tri, float* d_hit, void* hip_stream);
/* ANY (p->kind is ignored): d_occluded[i] = 1 if some triangle is accepted with t < t_max, else 0.  A lane
 * stops at the first traversal step that leaves a hit; up to there the walk is the closest-hit walk, so
 * d_occluded[i] == (d_tri[i] >= 0) of mcpt_trace_device for the same ray and t_max. */
int mcpt_occluded_device(mcpt_scene*, const mcpt_trace_params* p, int64_t n, const float* d_o, const float* d_d,
                         const float* d_t_max, uint8_t* d_occluded, void* hip_stream);
/* host arrays, synchronous; stats may be NULL (rays, inner/leaf visits, leaf refs, tri tests, spills of
 * this call; the counters mcpt_trace_stats_read reports are not touched) */
int mcpt_occluded(mcpt_scene*, const mcpt_trace_params* p, int64_t n, const float* o, const float* d,
                  const float* t_max, uint8_t* occluded, mcpt_render_stats* stats);
/* counters of the device ray queries since the last read; waits for them and resets.  The render stats
 * (mcpt_render_stats_read) are never touched by a ray query, and the other way round. */
int mcpt_trace_stats_read(mcpt_scene*, mcpt_render_stats* out);
/* allocate what ray queries need (above), so that the device entries allocate nothing afterwards */
int mcpt_scene_reserve_rays(mcpt_scene*);

/* ---- device radiance queries: path-traced radiance over ray buffers ---------- */
/* The third query kind: for every ray of a device buffer, the mean of spp
 * path-traced samples of the radiance arriving along it -- the renders' path
 * loop (CVMCTracer mode: max_depth scatters and the terminal query), samplers,
 * RNG and traversal, started from the caller's rays instead of the pinhole
 * camera.  Directions are used exactly as given (not re-normalized; the BSDF
 * arithmetic assumes unit length: unlike the hit queries, which take any
 * length, a radiance query wants unit directions).  Otherwise preconditions
 * as mcpt_trace_device.
 * Ray i has the stream id id_i = d_stream[i], or i without d_stream.  Sample s
 * (global index spp_offset + s) starts from rng_init(id_i, TEA16(seed),
 * spp_offset + s), draws and drops the two uniforms a render spends on its
 * primary ray's jitter, then runs the render's loop: a ray that is the primary
 * ray of sample spp_offset + s of pixel id_i traces that render's path, draw
 * for draw.  Samples are summed in sample order inside chunks of spp_chunk, the
 * chunk sums in chunk order, divided by (float)spp; prev_count > 0 applies the
 * renders' linear running mean to the old content of the output.  Scheduling
 * (workgroups, ready_thresh, the layout) never changes a result.
 * The mode is a render parameter, not the scene's: a scene that also serves
 * QuinEngine renders answers radiance queries in CVMCTracer mode like any other.
 * Checks, before anything is launched or allocated and in this order:
 * MCPT_E_INVALID for a NULL scene, n < 0, a NULL required pointer with n > 0, a
 * field of the params out of range (the message names it); MCPT_E_UNSUPPORTED
 * for n >= 2^31 / 3 or n x chunks >= 2^31; MCPT_E_INVALID for a host-only scene
 * and for an output that overlaps an input.  n = 0 is a no-op.  A multi-device
 * scene runs the query on devices[0].  Not offered:
 * QuinEngine mode, batches sharded over devices.  The wavefront form:
 * mcpt_radiance_ex[_device], below.
 * Workspace, the scene's: the renders' stack spill area (run the queries on the
 * stream of the scene's renders, or synchronize), 16 B per (ray, chunk) of
 * partial sums, the tail samples' buffer and a work-unit counter.  After
 * mcpt_scene_reserve_radiance(p, n) or a first call, a call that needs no more
 * allocates nothing; growth on a capturing stream is MCPT_E_NOMEM.           */
typedef struct {
    uint32_t spp;          /* samples per ray this call; >= 1 */
    uint32_t spp_offset;   /* first global sample index; spp_offset + spp <= 2^32 */
    uint32_t spp_chunk;    /* samples per partial sum, 0 = spp */
    int32_t  max_depth;    /* scatter events, 0..1000 */
    float    illum;        /* emitter scale (ILLUM), finite */
    int32_t  fresnel_kd;   /* as mcpt_render_params */
    uint64_t seed;
    uint32_t prev_count;   /* running mean over calls; the output is read when > 0 */
    int32_t  lean;         /* 1: rays only are counted */
    int32_t  workgroups;   /* scheduling only: 0 = automatic, > 0 = at most this many */
    int32_t  ready_thresh; /* scheduling only: 0 = the megakernel's default for the layout, else 1..64 */
} mcpt_radiance_params;
void mcpt_radiance_params_default(mcpt_radiance_params*);   /* spp 1, max_depth 7, illum 10, fresnel_kd 1, the renders' seed */

/* d_o, d_d: n*3 floats each; d_stream: n stream ids or NULL; d_radiance: n*4 floats (r, g, b, 0), read first
 * when p->prev_count > 0.  Asynchronous on hip_stream.  p may be NULL (the defaults).  The eight counters of
 * the call (paths and shades among them) are added to the block mcpt_trace_stats_read reports. */
int mcpt_radiance_device(mcpt_scene*, const mcpt_radiance_params* p, int64_t n, const float* d_o, const float* d_d,
                         const uint32_t* d_stream, float* d_radiance, void* hip_stream);
/* host arrays, synchronous; radiance: n*3 floats (read first when p->prev_count > 0); stats may be NULL (the
 * counters of this call; the block mcpt_trace_stats_read reports and the render stats are not touched) */
int mcpt_radiance(mcpt_scene*, const mcpt_radiance_params* p, int64_t n, const float* o, const float* d,
                  const uint32_t* stream, float* radiance, mcpt_render_stats* stats);
/* allocate what a radiance query of n rays with these params needs (above) */
int mcpt_scene_reserve_radiance(mcpt_scene*, const mcpt_radiance_params* p, int64_t n);

/* ---- radiance queries on either pipeline ---------------------------------------- */
/* The radiance queries with the pipeline as a parameter.  pipeline =
 * MCPT_PIPELINE_MEGAKERNEL (the default; p = NULL means the defaults) is exactly
 * mcpt_radiance[_device]: same code path, same bits, same counters.
 * MCPT_PIPELINE_WAVEFRONT runs the rays as a wavefront render of n "pixels": a
 * generate kernel fills the first ray queue from the buffers, bounce 0's extend
 * reads its origins from that queue, and every later kernel, route and cull is the
 * wavefront renders' (miss cull, direct lists and resolve, clip walk, sphere clip,
 * terminal cull, the co-resident shade).  Semantics, preconditions, accumulation,
 * the running mean, stream ids and the output layout are mcpt_radiance[_device]'s,
 * and the result is bit for bit what the megakernel form writes for the same rays
 * and `base`; the pipeline, batch split, streams, refill, group shift, sort and
 * layout never change a result.
 * Checks: mcpt_radiance's up to the work-unit limit, in its order; then the
 * wavefront fields with the ranges and messages of mcpt_render_params
 * (MCPT_E_INVALID, the message names the field); then the host-only scene and the
 * overlap check.  All before anything is launched or allocated.
 * Counters: the device entry adds its eight counters to the block
 * mcpt_trace_stats_read reports, the host entry reports its own call and leaves
 * that block alone.  On the wavefront a lean query counts rays, paths and shades
 * and its traversal counters read 0 (the wavefront renders' rule, not the lean
 * megakernel's); a counting query reports the megakernel query's counters, and the
 * host entry's stats->variant is 4 (scene in LDS) or 5 (in global memory).  The
 * render stats, mcpt_scene_direct_rays and its siblings and
 * mcpt_scene_primary_tile_classes are never touched by a query.
 * Workspace, wavefront: the scene's wavefront workspace (queues, partial sums,
 * spill areas, side streams), shared with the renders and planned as for a frame of
 * n pixels x spp -- run the queries on the stream of the scene's renders, or
 * synchronize -- plus the queries' counter blocks.  After
 * mcpt_scene_reserve_radiance_ex(p, n) a query that needs no more allocates
 * nothing; on a capturing stream the wavefront form follows a wavefront
 * mcpt_render_device: growth there is MCPT_E_NOMEM before any launch.  A
 * multi-device scene answers on devices[0].
 * A wavefront reservation bounds the default batches of later queries as
 * mcpt_scene_reserve's bounds a render's: reserve for the largest query.
 * Measured at 16 spp, lean ("The wavefront form"): the
 * wavefront form takes 0.52x the megakernel form's time on scene01 at 2^22 rays and
 * 0.73x at 2^20, 0.62x on the 70k mesh at both.  It does not win at 2^16 rays
 * (2^20 paths): there a query is a few dozen launches of ~1 ms in all, and the
 * wavefront form takes 2.0x (scene01) and 2.7x (70k mesh) the megakernel's time --
 * small batches belong on the megakernel. */
typedef struct {
    mcpt_radiance_params base;   /* as mcpt_radiance*; workgroups and ready_thresh are checked, and ignored on the wavefront */
    int32_t  pipeline;           /* MCPT_PIPELINE_*; megakernel (0): exactly mcpt_radiance[_device] */
    uint32_t wf_batch;           /* as mcpt_render_params: max paths per batch and stream, 0 = automatic */
    int32_t  wf_streams, wf_refill, wf_group_shift, wf_sort;   /* as mcpt_render_params, 0 = its defaults */
    uint64_t wf_mem_limit;       /* as mcpt_render_params */
} mcpt_radiance_ex_params;
void mcpt_radiance_ex_params_default(mcpt_radiance_ex_params*);   /* base: mcpt_radiance_params_default; the rest 0 */
int mcpt_radiance_ex_device(mcpt_scene*, const mcpt_radiance_ex_params*, int64_t n, const float* d_o, const float* d_d,
                            const uint32_t* d_stream, float* d_radiance, void* hip_stream);
int mcpt_radiance_ex(mcpt_scene*, const mcpt_radiance_ex_params*, int64_t n, const float* o, const float* d,
                     const uint32_t* stream, float* radiance, mcpt_render_stats* stats);
int mcpt_scene_reserve_radiance_ex(mcpt_scene*, const mcpt_radiance_ex_params*, int64_t n);
/* {direct, extend, clipped, sphere_skips} rays of the wavefront radiance queries in the record
   mcpt_trace_stats_read last read (zeros for megakernel queries and the hit queries) */
int mcpt_scene_query_route_rays(const mcpt_scene*, uint64_t out[4]);

/* ---- ambient-occlusion queries: hemisphere visibility of points and of pixels ---- */
/* Between the hit queries and the radiance queries: for every point, the share
 * of spp cosine-hemisphere rays of length `radius` that reach nothing (1 = open).
 * The library makes the rays -- the renders' RNG, hemisphere sampler and origin
 * rule -- and walks them with mcpt_occluded_device's any-hit walk; no buffer of
 * rays or flags exists.  All float arithmetic is fp32, one rounding per
 * operation.  CVMCTracer mode.
 * Point form (mcpt_ao[_device]): points p_i and normals n_i (unit length, used
 * as given), stream id id_i = d_stream[i], or i without d_stream.  Sample s of
 * point i, s in [0, spp): sd = rng_init(id_i, TEA16(seed), spp_offset + s), the
 * renders' and the radiance queries' stream; two uniforms are drawn and dropped
 * (a render's jitter, as mcpt_radiance_device); x, y the next two; h = the
 * renders' hemisphere sample of (x, y) about n_i (the reference's sampleHemi);
 * origin p_i + bias * h, direction h; the sample is occluded iff
 * mcpt_occluded_device answers 1 for that ray with t_max = radius.
 * Pixel form (mcpt_render_ao[_device]): sample s of pixel (px, py) of a frame is
 * the render's primary ray of sample spp_offset + s -- same stream, jitter and
 * reprojection as the renders and mcpt_render_aov -- and its closest hit.  A miss
 * counts as unoccluded and traces no second ray.  A hit forms what a render's
 * diffuse scatter forms there, whatever the material (emitters, glass and Phong
 * alike; the material is not read): the normalized shading normal nrm, flip =
 * dot(d, nrm) > 0, h = the hemisphere sample of the stream's next two draws
 * about nrm, dir = flip ? -h : h, origin (o + t * d) + 0.01 * dir; then the
 * any-hit walk with t_max = radius.
 * Value: v = (float)unoccluded / (float)spp; with prev_count > 0 the output is
 * read first and (old * (float)prev_count + v) / (float)(prev_count + 1) is
 * written (the feature buffers' linear running mean).  The unoccluded samples
 * are counted in integers, so the scheduling fields, the layout and any split of
 * a point's samples over lanes never change a bit.
 * The pixel form reads width, height, spp, spp_offset, seed, prev_count, fov_deg,
 * eye, dir, up and tile from the render params (the rest is ignored, as
 * mcpt_render_aov does) and only radius, lean, workgroups, refill and
 * unit_samples from the AO params: their spp, spp_offset, bias, seed and
 * prev_count are checked and otherwise ignored.
 * Checks, before anything is launched or allocated and in this order:
 * MCPT_E_INVALID for a NULL scene, n < 0, a NULL required pointer with n > 0, a
 * field out of range (the message names it); MCPT_E_UNSUPPORTED for n (or width x
 * height) >= 2^31 / 3, and in the pixel form for QuinEngine mode, shard_count > 1
 * and packed; MCPT_E_INVALID for a host-only scene and for an output that
 * overlaps an input.  n = 0 is a no-op.  A multi-device scene answers on
 * devices[0].  Not offered: distance-weighted falloff,
 * QuinEngine mode, batches sharded over devices.
 * Counters: the device entries add to the block mcpt_trace_stats_read reports, the
 * host entries report their own call and leave that block alone; the render stats
 * are never touched.  paths = samples started, shades = samples that formed an
 * occlusion ray (point form: all; pixel form: the primary hits), rays = every ray
 * walked (pixel form: primary and occlusion rays); the traversal counters are the
 * sum of the walks, and read 0 on a lean call.
 * Workspace, the scene's, O(n): the renders' stack spill area (run the queries on
 * the stream of the scene's renders, or synchronize), the ray queries' counter
 * blocks and 4 B per point or pixel.  After mcpt_scene_reserve_ao(n) or a first
 * call, a call that needs no more allocates nothing; growth on a capturing
 * stream is MCPT_E_NOMEM before any launch.                                   */
typedef struct {
    uint32_t spp;          /* samples per point this call; >= 1 */
    uint32_t spp_offset;   /* first global sample index; spp_offset + spp <= 2^32 */
    float    radius;       /* t_max of every occlusion ray; 0 = FLT_MAX (unbounded); >= 0, not NaN */
    float    bias;         /* point form: origin = p + bias * dir; 0 = 0.01 (the renders' literal); > 0, finite */
    uint64_t seed;
    uint32_t prev_count;   /* running mean over calls; the output is read when > 0 */
    int32_t  lean;         /* 1: traversal counters compiled out (rays, paths, shades still counted) */
    int32_t  workgroups;   /* scheduling only, as mcpt_trace_params */
    int32_t  refill;       /* scheduling only, 0 or 1..64 */
    int32_t  unit_samples; /* scheduling only: samples of one point a lane takes as one work unit; 0 = automatic */
} mcpt_ao_params;
void mcpt_ao_params_default(mcpt_ao_params*);   /* spp 1, the renders' seed, rest 0 */

/* d_p, d_n: n*3 floats each; d_stream: n stream ids or NULL; d_ao: n floats, read first when p->prev_count > 0.
 * Asynchronous on hip_stream.  p may be NULL (the defaults). */
int mcpt_ao_device(mcpt_scene*, const mcpt_ao_params* p, int64_t n, const float* d_p, const float* d_n,
                   const uint32_t* d_stream, float* d_ao, void* hip_stream);
/* host arrays, synchronous; ao: n floats (read first when p->prev_count > 0); stats may be NULL (the counters of
 * this call) */
int mcpt_ao(mcpt_scene*, const mcpt_ao_params* p, int64_t n, const float* p_xyz, const float* nrm,
            const uint32_t* stream, float* ao, mcpt_render_stats* stats);
/* d_ao: width*height floats, row-major, read first when rp->prev_count > 0.  Asynchronous on hip_stream.  ap may be
 * NULL (the defaults); rp may not. */
int mcpt_render_ao_device(mcpt_scene*, const mcpt_render_params* rp, const mcpt_ao_params* ap, float* d_ao,
                          void* hip_stream);
/* host array, synchronous; stats may be NULL (the counters of this call) */
int mcpt_render_ao(mcpt_scene*, const mcpt_render_params* rp, const mcpt_ao_params* ap, float* ao,
                   mcpt_render_stats* stats);
/* allocate what a query of n points, or a frame of n pixels, needs (above) */
int mcpt_scene_reserve_ao(mcpt_scene*, int64_t n_points_or_pixels);

/* ---- direct-lighting queries: emitter light at points and at pixels ---- */
/* The fourth query kind: for every point x with unit normal n, the cosine-weighted
 * mean of the emitter radiance over the hemisphere about n (E / pi), estimated by
 * area sampling of the scene's emitters.  A diffuse surface's direct radiance is Kd
 * times the value (mcpt_render_aov's albedo); a render's diffuse scatter followed by a
 * terminal query converges to the same quantity.  All device arithmetic is fp32, one
 * rounding per operation, no contraction.  CVMCTracer mode.
 * Light table, built by mcpt_scene_create* (host-only scenes too): a light triangle
 * is a kd triangle id k whose geometry is an emitter (some Ka > 0) and whose area is
 * above 0, in ascending kd id; v0, v1, v2 its fp32 vertices (mcpt_scene_copy_kd's).
 * In double, no fused multiply-add: e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2, len =
 * sqrt((c.x*c.x + c.y*c.y) + c.z*c.z), a_k = 0.5 * len, ng_k = (float)(c / len);
 * S_k = S_(k-1) + a_k in table order, A_tot = (float)S_last, cdf_k = (float)(S_k /
 * S_last): the last entry is 1.0f exactly.  A uniform u selects j = min(#{k : cdf_k <=
 * u}, L - 1): the first entry with u < cdf_j, or the last.
 * One sample, from x, n, bias and an RNG state sd that has spent two draws:
 * u0, u1, u2 = rng_next(sd); j from u0; su = sqrt(u1), beta = su * (1 - u2), gamma =
 * su * u2; y = (v0 * (1 - beta - gamma) + v1 * beta) + v2 * gamma; w = y - x, r2 =
 * dot(w, w), r = sqrt(r2), dir = w / r; cx = dot(n, dir), cy = |dot(ng_j, dir)|
 * (emitters radiate from both sides, as in the renders).  Unless cx > 0, cy > 0 and
 * r > 2 * bias the sample adds (0, 0, 0) and walks nothing.  Else the shadow ray has
 * origin x + dir * bias, direction dir and t_max = r - 2 * bias, and is occluded iff
 * mcpt_occluded_device answers 1 for it; an unoccluded sample adds g * (Ka[c] *
 * illum) per channel c, Ka of triangle j's geometry, g = ((cx * cy) * A_tot) /
 * (kPwPi * r2), kPwPi = 3.14159265359f.
 * Accumulation (as the radiance queries): the samples are added in sample order
 * inside chunks of spp_chunk (0 = spp), the chunk sums in chunk order from 0, the
 * total divided by (float)spp; with prev_count > 0 the output is read first and (old *
 * (float)prev_count + v) / (float)(prev_count + 1) written.  spp_chunk is part of the
 * result's definition; workgroups, refill and the scene's layout never change a bit.
 * Point form (mcpt_direct[_device]): points p_i, unit normals n_i (used as given),
 * stream id id_i = d_stream[i], or i without d_stream.  Sample s: sd = rng_init(id_i,
 * TEA16(seed), spp_offset + s), two uniforms drawn and dropped (a render's jitter, as
 * mcpt_ao_device), then the sample above at x = p_i, n = n_i.
 * Pixel form (mcpt_render_direct[_device]): sample s of pixel (px, py) is the render's
 * primary ray of sample spp_offset + s (mcpt_render_aov's and mcpt_render_ao's) and
 * its closest hit.  A miss adds zeros.  At a hit, whatever the material (emitters,
 * glass and Phong alike; the material is not read): nrm the normalized shading
 * normal, n = dot(d, nrm) > 0 ? -nrm : nrm, x = o + t * d, bias the literal 0.01, and
 * the stream's next three draws go to the sample above.  The render params give the
 * fields mcpt_render_ao_device reads; the direct params give spp_chunk, illum, lean,
 * workgroups and refill: their spp, spp_offset, bias, seed and prev_count are checked
 * and otherwise ignored.
 * Checks, before anything is launched or allocated and in this order: MCPT_E_INVALID
 * for a NULL scene, n < 0, a NULL required pointer with n > 0, a field out of range
 * (the message names it; illum not finite, bias negative, NaN or infinite);
 * MCPT_E_UNSUPPORTED for n (or width x height) >= 2^31 / 3, for n x chunks >= 2^31,
 * and in the pixel form for QuinEngine mode, shard_count > 1 and packed;
 * MCPT_E_INVALID for a host-only scene and for an output that overlaps an input.
 * n = 0 is a no-op.  A scene without a light triangle launches no walk: zeros, or the
 * running mean of zeros, are written.  A multi-device scene answers on devices[0].
 * Not offered: QuinEngine mode, batches sharded over devices,
 * multiple importance sampling with the BSDF, power- or distance-weighted light
 * selection, use inside the renders' path loop.
 * Counters (as the ambient-occlusion queries): the device entries add to the block
 * mcpt_trace_stats_read reports, the host entries report their own call; the render
 * stats are never touched.  paths = samples started, shades = samples that formed a
 * shadow ray, rays = every ray walked (pixel form: primary and shadow rays); the
 * traversal counters are the sum of the walks, and read 0 on a lean call.
 * Workspace, the scene's: the renders' stack spill area (run the queries on the
 * stream of the scene's renders, or synchronize), the ray queries' counter blocks,
 * the light table (64 B and a cdf entry per light, uploaded with the scene) and, with
 * more than one chunk, 16 B per (point or pixel, chunk).  After
 * mcpt_scene_reserve_direct or a first call, a call that needs no more allocates
 * nothing; growth on a capturing stream is MCPT_E_NOMEM before any launch.        */
typedef struct {
    uint32_t spp;          /* samples per point this call; >= 1 */
    uint32_t spp_offset;   /* first global sample index; spp_offset + spp <= 2^32 */
    uint32_t spp_chunk;    /* samples per partial sum; 0 = spp (one chunk); part of the result */
    float    illum;        /* the emitters' scale (a render's illum); finite */
    float    bias;         /* point form: shadow rays start at x + bias * dir; 0 = 0.01; >= 0, finite */
    uint64_t seed;
    uint32_t prev_count;   /* running mean over calls; the output is read when > 0 */
    int32_t  lean;         /* 1: traversal counters compiled out (rays, paths, shades still counted) */
    int32_t  workgroups;   /* scheduling only, as mcpt_trace_params */
    int32_t  refill;       /* scheduling only, 0 or 1..64 */
} mcpt_direct_params;
void mcpt_direct_params_default(mcpt_direct_params*);   /* spp 1, illum 10, the renders' seed, rest 0 */

/* The light table: returns the number of lights L; each pointer may be NULL.  kd_ids: L
 * kd triangle ids, ascending; cdf: L floats; normals: L*3 floats; area_total: A_tot.
 * Works on host-only scenes; 0 for a NULL scene. */
int mcpt_scene_lights(const mcpt_scene*, int32_t* kd_ids, float* cdf, float* normals, float* area_total);

/* d_p, d_n: n*3 floats each; d_stream: n stream ids or NULL; d_out: n*4 floats (r, g, b, 0), read first when
 * p->prev_count > 0.  Asynchronous on hip_stream.  p may be NULL (the defaults). */
int mcpt_direct_device(mcpt_scene*, const mcpt_direct_params* p, int64_t n, const float* d_p, const float* d_n,
                       const uint32_t* d_stream, float* d_out, void* hip_stream);
/* host arrays, synchronous; out: n*3 floats (read first when p->prev_count > 0); stats may be NULL (the counters
 * of this call) */
int mcpt_direct(mcpt_scene*, const mcpt_direct_params* p, int64_t n, const float* p_xyz, const float* nrm,
                const uint32_t* stream, float* out, mcpt_render_stats* stats);
/* d_out_rgba: width*height*4 floats (r, g, b, 0), row-major, read first when rp->prev_count > 0.  Asynchronous on
 * hip_stream.  dp may be NULL (the defaults); rp may not. */
int mcpt_render_direct_device(mcpt_scene*, const mcpt_render_params* rp, const mcpt_direct_params* dp,
                              float* d_out_rgba, void* hip_stream);
/* host array of width*height*3 floats, synchronous; stats may be NULL (the counters of this call) */
int mcpt_render_direct(mcpt_scene*, const mcpt_render_params* rp, const mcpt_direct_params* dp, float* out,
                       mcpt_render_stats* stats);
/* allocate what a query of n points, or a frame of n pixels, with p's spp and spp_chunk needs (above); p may be
 * NULL (one chunk) */
int mcpt_scene_reserve_direct(mcpt_scene*, const mcpt_direct_params* p, int64_t n_points_or_pixels);

#ifdef __cplusplus
}
#endif
#endif /* MCPT_H */
