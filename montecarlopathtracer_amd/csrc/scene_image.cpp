// scene_image.cpp -- models and scenes of the C ABI (include/mcpt.h): the model
// descriptors, the device image of a scene (CreateGeometry of the reference's
// PW::Tracer module, CVMCTracer/CUDA/CUTracer.cu:220-404), its upload to one
// device or several, teardown (DestroyGeometry, here freeing exactly what was
// allocated) and the entries that report what a scene holds.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "capi_internal.hpp"
#include "half_box.hpp"

using namespace mcpt::host;

mcpt_scene::~mcpt_scene() {
    if (!on_device) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    destroy_comms(*this);
    for (DevBuf* b : buffers())
        if (b->p) (void)hipFree(b->p);
    if (ad_host_n) (void)hipHostFree(ad_host_n);
    for (void* p : retired) (void)hipFree(p);
    for (auto& t : pending) for (auto ev : t.e) (void)hipEventDestroy(ev);
    for (auto& t : free_timing) for (auto ev : t.e) (void)hipEventDestroy(ev);
    if (has_capture_timing) for (auto ev : capture_timing.e) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {done, start, wf_fork})
        if (ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < mcpt::kMaxWfStreams; i++) {
        if (wf_join[i]) (void)hipEventDestroy(wf_join[i]);
        if (wf_stream[i]) (void)hipStreamDestroy(wf_stream[i]);
    }
    if (stream) (void)hipStreamDestroy(stream);
    replicas.clear();                 // each replica frees on its own device
    if (prev >= 0) (void)hipSetDevice(prev);
}

namespace {

// Device node order: treelet clusters.  A cluster holds the sibling pairs of
// the 3 levels below its root (<= 7 pairs) contiguously, so a descent through
// those levels stays within 112 B (16-B pairs, LDS scenes) or 336 B (48-B
// pair records with child boxes, global-memory scenes); clusters are emitted
// breadth-first (the top of the tree comes first).  Slot 0 is padding and
// slot 1 the root.  Triangles and leaf references are renumbered in the order
// the leaves appear, so a leaf's triangles sit near its neighbours'.  Only
// addresses change: traversal order, results and counters are those of the
// BFS tree.
struct DeviceOrder {
    std::vector<uint32_t> node_new;     // host node -> device node index
    uint32_t n_slots = 0;               // device node indices in use (incl. padding)
    std::vector<uint32_t> leaf_order;   // host leaf nodes in device order
    std::vector<uint32_t> tri_order;    // device triangle slot -> kd id
    std::vector<uint32_t> tri_new;      // kd id -> device triangle slot
};

// leaves in device node order, triangles by first appearance
void order_leaves(const mcpt::HostScene& hs, DeviceOrder& d) {
    const uint32_t nn = static_cast<uint32_t>(hs.nodes.size());
    std::vector<uint32_t> by_dev(d.n_slots, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < nn; ++i) by_dev[d.node_new[i]] = i;
    d.tri_new.assign(hs.kd_tris.size(), 0xFFFFFFFFu);
    for (uint32_t dv = 0; dv < d.n_slots; ++dv) {
        const uint32_t i = by_dev[dv];
        if (i == 0xFFFFFFFFu || hs.nodes[i].axis) continue;
        d.leaf_order.push_back(i);
        for (uint32_t r = 0; r < hs.nodes[i].leaf_count; ++r) {
            const uint32_t k = hs.leaf_ids[hs.nodes[i].leaf_begin + r];
            if (d.tri_new[k] == 0xFFFFFFFFu) {
                d.tri_new[k] = static_cast<uint32_t>(d.tri_order.size());
                d.tri_order.push_back(k);
            }
        }
    }
    for (uint32_t k = 0; k < d.tri_new.size(); ++k)
        if (d.tri_new[k] == 0xFFFFFFFFu) {
            d.tri_new[k] = static_cast<uint32_t>(d.tri_order.size());
            d.tri_order.push_back(k);
        }
}

DeviceOrder device_order(const mcpt::HostScene& hs) {
    const uint32_t nn = static_cast<uint32_t>(hs.nodes.size());
    DeviceOrder d;
    d.node_new.assign(nn, 0xFFFFFFFFu);
    d.node_new[0] = 0;
    uint32_t pairs = 0;                  // pair m occupies device nodes 2m+1, 2m+2 (slots 2m+2, 2m+3)
    std::vector<uint32_t> queue{0}, list, frontier, next;
    for (size_t qi = 0; qi < queue.size(); ++qi) {
        list.clear();
        frontier.assign(1, queue[qi]);
        for (int lvl = 0; lvl < 3; ++lvl) {
            next.clear();
            for (uint32_t n : frontier)
                if (hs.nodes[n].axis) {
                    list.push_back(hs.nodes[n].left);
                    next.push_back(hs.nodes[n].left);
                    next.push_back(hs.nodes[n].left + 1);
                }
            frontier.swap(next);
        }
        for (uint32_t n : frontier)
            if (hs.nodes[n].axis) queue.push_back(n);
        if (list.empty()) continue;
        for (uint32_t L : list) {
            d.node_new[L] = 2 * pairs + 1;
            d.node_new[L + 1] = 2 * pairs + 2;
            ++pairs;
        }
    }
    d.n_slots = 2 * pairs + 1;
    order_leaves(hs, d);
    return d;
}

void build_image(mcpt_scene& s, bool force_global) {
    const mcpt::HostScene& hs = s.hs;
    const uint32_t nt = static_cast<uint32_t>(hs.kd_tris.size());
    const uint32_t nn = static_cast<uint32_t>(hs.nodes.size());
    const uint32_t nl = static_cast<uint32_t>(hs.leaf_ids.size());
    const uint32_t ng = static_cast<uint32_t>(hs.geoms.size());
    // the traversal's spill area holds 32 stack entries per lane (depth cap 32: kSpillEntries)
    if (hs.kd_depth < 0 || hs.kd_depth > static_cast<int>(kSpillEntries))
        throw mcpt::Error{MCPT_E_INVALID, "KD tree deeper than 32"};
    for (uint32_t i = 0; i < nn; ++i)
        if (hs.nodes[i].axis && ((hs.nodes[i].left % 2u) != 1u || hs.nodes[i].right != hs.nodes[i].left + 1u ||
                                 hs.nodes[i].left + 1u >= nn || hs.nodes[i].left <= i))
            throw mcpt::Error{MCPT_E_INVALID, "KD sibling pair not at an odd index"};
    auto al16 = [](size_t x) { return (x + 15u) & ~size_t(15); };
    auto al128 = [](size_t x) { return (x + 127u) & ~size_t(127); };
    // Scenes that fit in LDS: 8-B node records in packed cluster order (every
    // LDS byte counts).  Larger scenes: 48-B sibling-pair records -- the two
    // node words plus both children's KD boxes as fp16 rounded outward, so the
    // traversal skips children the ray misses (child-box cull).
    DeviceOrder ord = device_order(hs);
    bool boxes = false;
    auto image_size = [&](const DeviceOrder& o, size_t& on, size_t& ol, size_t& og) {
        on = al128(size_t(nt) * 48);
        if (boxes) ol = al16(on + size_t((o.n_slots - 1) / 2) * 48);   // pair m: device nodes 2m+1, 2m+2
        else ol = al16(on + size_t(o.n_slots + 1) * 8);                 // node slot j = device node j-1
        og = al16(ol + size_t(nl) * 4);
        // (geometries never empty for a scene with triangles; the paired
        // triangle tests read the ref after a leaf's last one, so the leaf
        // section must never end the image)
        return al16(og + size_t(std::max<uint32_t>(ng, 1u)) * 64);
    };
    size_t off_nodes, off_leafs, off_geoms;
    size_t total = image_size(ord, off_nodes, off_leafs, off_geoms);
    // where the scene lives, decided here alone (scene_in_lds, render_launch.hpp, has the invariant)
    if (mcpt::lds_bytes_counted_in_lds(static_cast<uint32_t>(std::min<size_t>(total, 0xFFFFFFF0u)), 4) > mcpt::kMaxLds ||
        force_global) {
        boxes = true;
        total = image_size(ord, off_nodes, off_leafs, off_geoms);
    }
    const size_t off_tris = 0;
    if (total > 0xFFFFFFF0u) throw mcpt::Error{MCPT_E_UNSUPPORTED, "scene image exceeds 4 GiB"};
    if (ord.n_slots >= (1u << 29) || nl >= (1u << 30)) throw mcpt::Error{MCPT_E_UNSUPPORTED, "KD tree too large"};
    s.image.assign(total, 0);
    s.tri_order = ord.tri_order;
    unsigned char* img = s.image.data();
    for (uint32_t slot = 0; slot < nt; ++slot) {
        const uint32_t k = ord.tri_order[slot];
        const float* v = &hs.kd_verts[9 * size_t(k)];
        float rec[12] = {v[0], v[1], v[2], 0.0f,
                         v[0] - v[3], v[1] - v[4], v[2] - v[5], 0.0f,
                         v[0] - v[6], v[1] - v[7], v[2] - v[8], 0.0f};
        std::memcpy(&rec[3], &hs.kd_prio[k], 4);
        std::memcpy(&rec[7], &hs.kd_geom[k], 4);
        // the 2x2 minor (a-b).y (a-c).z - (a-c).y (a-b).z that Math.hpp:171-173's
        // det() forms for both A and tM (CUTracer.cu:72-83): ray-independent, so
        // stored once (same float operations as the kernel's, no contraction)
        rec[11] = rec[5] * rec[10] - rec[9] * rec[6];
        std::memcpy(img + off_tris + size_t(slot) * 48, rec, 48);
    }
    // leaf references, leaves in device order
    std::vector<uint32_t> leaf_begin_new(nn, 0);
    {
        uint32_t* refs = reinterpret_cast<uint32_t*>(img + off_leafs);
        uint32_t at = 0;
        for (uint32_t i : ord.leaf_order) {
            leaf_begin_new[i] = at;
            for (uint32_t r = 0; r < hs.nodes[i].leaf_count; ++r)
                refs[at++] = 3u * ord.tri_new[hs.leaf_ids[hs.nodes[i].leaf_begin + r]];   // record index
        }
    }
    for (uint32_t i = 0; i < nn; ++i) {
        const mcpt::KdNode& n = hs.nodes[i];
        uint32_t w[2];
        if (n.axis) {
            // LDS layout: the left child's device node index (its 8-B record
            // pair at slot index + 1); global layout: the 16-B offset 3m of the
            // children's 48-B pair record m (no index arithmetic per step)
            const uint32_t dl = ord.node_new[n.left];
            w[0] = ((n.axis - 1u) << 30) | (boxes ? 3u * ((dl - 1u) / 2u) : dl);
            std::memcpy(&w[1], &n.split, 4);
        } else {
            w[0] = (3u << 30) | leaf_begin_new[i];
            w[1] = n.leaf_count;
        }
        const uint32_t dv = ord.node_new[i];
        if (i == 0) {
            s.gpu.root_w[0] = w[0];
            s.gpu.root_w[1] = w[1];
            if (boxes) continue;              // the root has no pair record
        }
        if (!boxes) {
            std::memcpy(img + off_nodes + size_t(dv + 1) * 8, w, 8);
            continue;
        }
        // pair record: [w(left) w(right)] [box(left) box(right)] [pad]; boxes rounded outward
        const size_t m = (dv - 1) / 2, side = (dv - 1) % 2;
        unsigned char* rec = img + off_nodes + m * 48;
        std::memcpy(rec + side * 8, w, 8);
        uint16_t hb[6];
        for (int a = 0; a < 3; ++a) {
            hb[a] = mcpt::f32_to_f16_dir(n.bmin[a], -1);
            hb[3 + a] = mcpt::f32_to_f16_dir(n.bmax[a], +1);
        }
        std::memcpy(rec + 16 + side * 12, hb, 12);
    }
    for (uint32_t g = 0; g < ng; ++g) {
        const mcpt::Geometry& ge = hs.geoms[g];
        mcpt::GpuGeom gg{};
        gg.Ka[0] = ge.Ka.x; gg.Ka[1] = ge.Ka.y; gg.Ka[2] = ge.Ka.z;
        gg.Kd[0] = ge.Kd.x; gg.Kd[1] = ge.Kd.y; gg.Kd[2] = ge.Kd.z;
        gg.Ks[0] = ge.Ks.x; gg.Ks[1] = ge.Ks.y; gg.Ks[2] = ge.Ks.z;
        gg.Ns = ge.Ns; gg.Tr = ge.Tr; gg.Ni = ge.Ni;
        gg.Ns_u = ge.Ns > 0.0f ? (ge.Ns < 4294967040.0f ? static_cast<uint32_t>(ge.Ns) : 0xFFFFFF00u) : 0u;
        std::memcpy(img + off_geoms + size_t(g) * 64, &gg, 64);
    }
    mcpt::GpuScene& gs = s.gpu;
    gs.image_bytes = static_cast<uint32_t>(total);
    gs.off_tris = static_cast<uint32_t>(off_tris);
    gs.off_nodes = static_cast<uint32_t>(off_nodes);
    gs.off_leafs = static_cast<uint32_t>(off_leafs);
    gs.off_geoms = static_cast<uint32_t>(off_geoms);
    gs.node_boxes = boxes ? 1u : 0u;
    gs.n_tris = nt; gs.n_nodes = nn; gs.n_leafs = nl; gs.n_geoms = ng;
    if (nn) {
        for (int a = 0; a < 3; ++a) { gs.root_min[a] = hs.nodes[0].bmin[a]; gs.root_max[a] = hs.nodes[0].bmax[a]; }
    }
}

// The route tables of a scene (RouteTables, capi_internal.hpp) from its host scene
// and the image's triangle order (build_image): slot -> kd id
void route_tables(const mcpt::HostScene& hs, const std::vector<uint32_t>& tri_order, RouteTables& t) {
    const uint32_t nt = static_cast<uint32_t>(hs.kd_tris.size());
    // terminal cull: the emitter boxes, packed like a pair record's child box
    // (lo.x lo.y | lo.z hi.x | hi.y hi.z)
    float eb[mcpt::kMaxCullBoxes][6];
    t.n_cull_boxes = static_cast<uint32_t>(mcpt::terminal_cull_boxes(hs, eb, mcpt::kMaxCullBoxes));
    for (uint32_t b = 0; b < t.n_cull_boxes; ++b) {
        uint16_t hb[6];
        for (int a = 0; a < 3; ++a) {
            hb[a] = mcpt::f32_to_f16_dir(eb[b][a], -1);
            hb[3 + a] = mcpt::f32_to_f16_dir(eb[b][3 + a], +1);
        }
        std::memcpy(t.cull_box[b], hb, 12);
    }
    t.n_miss_boxes = static_cast<uint32_t>(mcpt::miss_cull_boxes(hs, t.miss_box, mcpt::kMaxMissBoxes));
    // direct lists: every triangle to one box that holds it; a box with 1..kDirectK
    // triangles is small and gets their record indices (the leaf refs' unit) in
    // image order.  (Kept for every scene with boxes; direct_lists_fit and the
    // render's kind decide whether a render uses them.)
    mcpt::direct_list_assign(hs, t.miss_box, static_cast<int>(t.n_miss_boxes), t.tri_box);
    t.direct_counts = 0;
    std::memset(t.direct_list, 0, sizeof t.direct_list);
    std::memset(t.box_tris, 0, sizeof t.box_tris);
    for (uint32_t slot = 0; slot < nt && t.n_miss_boxes; ++slot) {
        const int32_t b = t.tri_box[tri_order[slot]];
        if (b < 0) throw mcpt::Error{MCPT_E_INVALID, "a triangle outside every occluder box"};
        if (t.box_tris[b] < mcpt::kDirectK) t.direct_list[size_t(b) * mcpt::kDirectK + t.box_tris[b]] = 3u * slot;
        t.box_tris[b]++;
    }
    for (uint32_t b = 0; b < t.n_miss_boxes; ++b) {
        if (t.box_tris[b] >= 1 && t.box_tris[b] <= mcpt::kDirectK) t.direct_counts |= t.box_tris[b] << (4u * b);
        else std::memset(&t.direct_list[size_t(b) * mcpt::kDirectK], 0, 4 * mcpt::kDirectK);
    }
    // sphere clip: a sphere over the triangles of every box that has some and no list
    uint32_t unlisted = 0;
    for (uint32_t b = 0; b < t.n_miss_boxes; ++b)
        if (t.box_tris[b] > mcpt::kDirectK) unlisted |= 1u << b;
    t.clip_spheres = mcpt::clip_spheres(hs, t.miss_box, static_cast<int>(t.n_miss_boxes), t.tri_box, unlisted,
                                        mcpt::kSphereMargin, mcpt::kSphereMaxReach, t.clip_sphere);
    t.cull_gain = 0.0f;
    for (const mcpt::Geometry& ge : hs.geoms)
        for (float k : {ge.Kd.x, ge.Kd.y, ge.Kd.z, ge.Ks.x, ge.Ks.y, ge.Ks.z})
            if (std::fabs(k) > t.cull_gain) t.cull_gain = std::fabs(k);
}

// The light table as the direct-lighting kernels read it (direct_launch.hpp): one
// 64-B record per light -- the kd triangle's vertices with the normal's components in
// the fourth words, then the geometry's Ka -- and the cdf behind the records
std::vector<float> light_image(const mcpt::HostScene& hs, const mcpt::LightTable& t) {
    const size_t L = t.kd_ids.size();
    std::vector<float> img(L * 16 + L, 0.0f);
    for (size_t i = 0; i < L; ++i) {
        const size_t k = static_cast<size_t>(t.kd_ids[i]);
        const float* v = &hs.kd_verts[9 * k];
        const mcpt::Geometry& ge = hs.geoms[hs.kd_geom[k]];
        float* rec = &img[16 * i];
        for (int j = 0; j < 3; ++j) {
            for (int a = 0; a < 3; ++a) rec[4 * j + a] = v[3 * j + a];
            rec[4 * j + 3] = t.normals[3 * i + j];
        }
        rec[12] = ge.Ka.x; rec[13] = ge.Ka.y; rec[14] = ge.Ka.z;
        img[L * 16 + i] = t.cdf[i];
    }
    return img;
}

// device copies of the scene image, the shading normals and the light table on `device`
void upload(mcpt_scene& s, int device, const std::vector<unsigned char>& image, const std::vector<float>& nrm,
            const std::vector<float>& lights) {
    HIP_TRY(hipSetDevice(device));
    s.device = device;
    HIP_TRY(hipDeviceGetAttribute(&s.cus, hipDeviceAttributeMultiprocessorCount, s.device));
    s.on_device = true;
    HIP_TRY(hipMalloc(&s.d_image.p, image.size()));
    HIP_TRY(hipMemcpy(s.d_image.p, image.data(), image.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&s.d_normals.p, nrm.size() * 4));
    HIP_TRY(hipMemcpy(s.d_normals.p, nrm.data(), nrm.size() * 4, hipMemcpyHostToDevice));
    s.gpu.image = static_cast<const unsigned char*>(s.d_image.p);
    s.gpu.normals = static_cast<const float4*>(s.d_normals.p);
    if (!lights.empty()) {
        HIP_TRY(hipMalloc(&s.d_lights.p, lights.size() * 4));
        s.d_lights.bytes = lights.size() * 4;
        HIP_TRY(hipMemcpy(s.d_lights.p, lights.data(), lights.size() * 4, hipMemcpyHostToDevice));
    }
}

int scene_create_impl(const mcpt_model* m, mcpt_scene** out, bool device, const char* kd_cache_dir = nullptr,
                      int32_t* cache_hit = nullptr, int32_t layout = MCPT_LAYOUT_AUTO,
                      int32_t kd_build = MCPT_KD_BUILD_REFERENCE) {
    return guarded([&]() -> int {
        if (!m || !out) return fail(MCPT_E_INVALID, "NULL argument");
        if (kd_build != MCPT_KD_BUILD_REFERENCE && kd_build != MCPT_KD_BUILD_SAH)
            return fail(MCPT_E_INVALID, "unknown kd_build");
        auto s = std::make_unique<mcpt_scene>();
        int hit = 0;
        mcpt::build_host_scene(m->m, s->hs, kd_cache_dir, &hit, kd_build);
        if (cache_hit) *cache_hit = hit;
        if (s->hs.kd_tris.empty()) return fail(MCPT_E_INVALID, "scene has no triangles");
        if (layout != MCPT_LAYOUT_AUTO && layout != MCPT_LAYOUT_GLOBAL) return fail(MCPT_E_INVALID, "unknown layout");
        build_image(*s, layout == MCPT_LAYOUT_GLOBAL);
        route_tables(s->hs, s->tri_order, s->tables);
        mcpt::light_table(s->hs, s->lights);
        if (device) {
            const std::vector<float> lights = light_image(s->hs, s->lights);
            const size_t nt = s->hs.kd_tris.size();
            std::vector<float> nrm(nt * 12, 0.0f);
            for (size_t k = 0; k < nt; ++k)          // image triangle order
                for (int j = 0; j < 3; ++j)
                    for (int c = 0; c < 3; ++c)
                        nrm[12 * k + 4 * j + c] = s->hs.kd_normals[9 * size_t(s->tri_order[k]) + 3 * j + c];
            int cur = 0;
            HIP_TRY(hipGetDevice(&cur));
            const std::vector<int> devs = g_devices.empty() ? std::vector<int>{cur} : g_devices;
            upload(*s, devs[0], s->image, nrm, lights);
            // replicas for the further devices: same image, own workspace and stream
            for (size_t i = 1; i < devs.size(); ++i) {
                auto R = std::make_unique<mcpt_scene>();
                R->gpu = s->gpu;
                R->tables = s->tables;
                R->lights = s->lights;
                upload(*R, devs[i], s->image, nrm, lights);
                HIP_TRY(hipStreamCreateWithFlags(&R->stream, hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&R->done, hipEventDisableTiming));
                s->replicas.push_back(std::move(R));
            }
            HIP_TRY(hipSetDevice(devs[0]));
            s->peer_access = g_peer_ok;
        }
        *out = s.release();
        return MCPT_OK;
    });
}

}  // namespace

extern "C" {

int mcpt_model_create(const mcpt_model_desc* d, mcpt_model** out) {
    return guarded([&]() -> int {
        if (!d || !out) return fail(MCPT_E_INVALID, "NULL argument");
        if (d->n_vertices < 1 || d->n_normals < 1 || d->n_triangles < 1 || d->n_materials < 1 || d->n_groups < 0)
            return fail(MCPT_E_INVALID, "arrays must include the dummy element 0");
        if (!d->vertices || !d->normals || !d->triangles || !d->materials ||
            (d->n_groups > 0 && (!d->group_names || !d->group_offsets || !d->group_tris)))
            return fail(MCPT_E_INVALID, "NULL array");
        auto m = std::make_unique<mcpt_model>();
        mcpt::ObjModel& o = m->m;
        o.path = "<memory>";
        o.vertices.resize(size_t(d->n_vertices));
        for (int64_t i = 0; i < d->n_vertices; ++i)
            o.vertices[size_t(i)] = mcpt::Vec3{d->vertices[3 * i], d->vertices[3 * i + 1], d->vertices[3 * i + 2]};
        o.normals.resize(size_t(d->n_normals));
        for (int64_t i = 0; i < d->n_normals; ++i)
            o.normals[size_t(i)] = mcpt::Vec3{d->normals[3 * i], d->normals[3 * i + 1], d->normals[3 * i + 2]};
        o.n_texcoords = 1;
        o.triangles.resize(size_t(d->n_triangles));
        for (int64_t i = 0; i < d->n_triangles; ++i) {
            const int32_t* t = d->triangles + 10 * i;
            auto& dst = o.triangles[size_t(i)];
            for (int j = 0; j < 3; ++j) { dst.v[j] = t[j]; dst.t[j] = t[3 + j]; dst.n[j] = t[6 + j]; }
            dst.material = t[9];
            if (i > 0 && (t[9] < 0 || t[9] >= d->n_materials)) return fail(MCPT_E_INVALID, "material index out of range");
        }
        o.materials.resize(size_t(d->n_materials));
        for (int64_t i = 0; i < d->n_materials; ++i) {
            const double* q = d->materials + 12 * i;
            auto& mt = o.materials[size_t(i)];
            mt.Ka = mcpt::Vec3{float(q[0]), float(q[1]), float(q[2])};
            mt.Kd = mcpt::Vec3{float(q[3]), float(q[4]), float(q[5])};
            mt.Ks = mcpt::Vec3{float(q[6]), float(q[7]), float(q[8])};
            mt.Ns = q[9]; mt.Tr = q[10]; mt.Ni = q[11];
        }
        for (int64_t g = 0; g < d->n_groups; ++g) {
            const int64_t b = d->group_offsets[g], e = d->group_offsets[g + 1];
            if (b < 0 || e < b) return fail(MCPT_E_INVALID, "bad group offsets");
            auto& dst = o.groups[d->group_names[g] ? d->group_names[g] : ""];
            for (int64_t k = b; k < e; ++k) {
                if (d->group_tris[k] < 1 || d->group_tris[k] >= d->n_triangles)
                    return fail(MCPT_E_INVALID, "group triangle index out of range");
                dst.push_back(d->group_tris[k]);
            }
        }
        *out = m.release();
        return MCPT_OK;
    });
}

int mcpt_model_read_obj(const char* path, mcpt_model** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(MCPT_E_INVALID, "path/out is NULL");
        auto m = std::make_unique<mcpt_model>();
        mcpt::read_obj(path, m->m);
        *out = m.release();
        return MCPT_OK;
    });
}

int mcpt_model_read_obj_ex(const char* path, int32_t flavor, mcpt_model** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(MCPT_E_INVALID, "path/out is NULL");
        if (flavor != MCPT_OBJ_CVMCTRACER && flavor != MCPT_OBJ_TINYOBJ) return fail(MCPT_E_INVALID, "unknown flavor");
        auto m = std::make_unique<mcpt_model>();
        mcpt::read_obj(path, m->m, flavor);
        *out = m.release();
        return MCPT_OK;
    });
}

void mcpt_model_free(mcpt_model* m) { delete m; }

int mcpt_model_get_info(const mcpt_model* m, mcpt_model_info* out) {
    if (!m || !out) return fail(MCPT_E_INVALID, "NULL argument");
    out->n_vertices = static_cast<int64_t>(m->m.vertices.size());
    out->n_normals = static_cast<int64_t>(m->m.normals.size());
    out->n_texcoords = m->m.n_texcoords;
    out->n_triangles = static_cast<int64_t>(m->m.triangles.size());
    out->n_materials = static_cast<int64_t>(m->m.materials.size());
    out->n_groups = static_cast<int64_t>(m->m.groups.size());
    return MCPT_OK;
}

int mcpt_model_copy_vertices(const mcpt_model* m, float* out) {
    if (!m || !out) return fail(MCPT_E_INVALID, "NULL argument");
    for (size_t i = 0; i < m->m.vertices.size(); ++i) {
        out[3 * i] = m->m.vertices[i].x; out[3 * i + 1] = m->m.vertices[i].y; out[3 * i + 2] = m->m.vertices[i].z;
    }
    return MCPT_OK;
}

int mcpt_model_copy_normals(const mcpt_model* m, float* out) {
    if (!m || !out) return fail(MCPT_E_INVALID, "NULL argument");
    for (size_t i = 0; i < m->m.normals.size(); ++i) {
        out[3 * i] = m->m.normals[i].x; out[3 * i + 1] = m->m.normals[i].y; out[3 * i + 2] = m->m.normals[i].z;
    }
    return MCPT_OK;
}

int mcpt_model_copy_triangles(const mcpt_model* m, int32_t* out) {
    if (!m || !out) return fail(MCPT_E_INVALID, "NULL argument");
    for (size_t i = 0; i < m->m.triangles.size(); ++i) {
        const auto& t = m->m.triangles[i];
        for (int j = 0; j < 3; ++j) { out[10 * i + j] = t.v[j]; out[10 * i + 3 + j] = t.t[j]; out[10 * i + 6 + j] = t.n[j]; }
        out[10 * i + 9] = t.material;
    }
    return MCPT_OK;
}

int mcpt_model_copy_materials(const mcpt_model* m, double* out) {
    if (!m || !out) return fail(MCPT_E_INVALID, "NULL argument");
    for (size_t i = 0; i < m->m.materials.size(); ++i) {
        const auto& t = m->m.materials[i];
        double* o = out + 12 * i;
        o[0] = t.Ka.x; o[1] = t.Ka.y; o[2] = t.Ka.z; o[3] = t.Kd.x; o[4] = t.Kd.y; o[5] = t.Kd.z;
        o[6] = t.Ks.x; o[7] = t.Ks.y; o[8] = t.Ks.z; o[9] = t.Ns; o[10] = t.Tr; o[11] = t.Ni;
    }
    return MCPT_OK;
}

int mcpt_model_group(const mcpt_model* m, int64_t g, char* name_buf, int64_t name_cap, int64_t* n, int32_t* tris) {
    if (!m || g < 0 || g >= static_cast<int64_t>(m->m.groups.size())) return fail(MCPT_E_INVALID, "bad group index");
    auto it = m->m.groups.begin();
    std::advance(it, g);
    if (name_buf && name_cap > 0) std::snprintf(name_buf, static_cast<size_t>(name_cap), "%s", it->first.c_str());
    if (n) *n = static_cast<int64_t>(it->second.size());
    if (tris && !it->second.empty()) std::memcpy(tris, it->second.data(), it->second.size() * sizeof(int32_t));
    return MCPT_OK;
}

int mcpt_scene_create(const mcpt_model* m, mcpt_scene** out) { return scene_create_impl(m, out, true); }
int mcpt_scene_create_host(const mcpt_model* m, mcpt_scene** out) { return scene_create_impl(m, out, false); }
int mcpt_scene_create_cached(const mcpt_model* m, const char* kd_cache_dir, int32_t host_only, mcpt_scene** out,
                             int32_t* cache_hit) {
    return scene_create_impl(m, out, host_only == 0, kd_cache_dir, cache_hit);
}
int mcpt_scene_create_ex(const mcpt_model* m, const mcpt_scene_options* o, mcpt_scene** out, int32_t* cache_hit) {
    const mcpt_scene_options d{nullptr, 0, MCPT_LAYOUT_AUTO, MCPT_KD_BUILD_REFERENCE};
    if (!o) o = &d;
    const char* dir = o->kd_cache_dir && o->kd_cache_dir[0] ? o->kd_cache_dir : nullptr;
    return scene_create_impl(m, out, o->host_only == 0, dir, cache_hit, o->layout, o->kd_build);
}

void mcpt_scene_destroy(mcpt_scene* s) { delete s; }

int mcpt_scene_get_info(const mcpt_scene* s, mcpt_scene_info* out) {
    if (!s || !out) return fail(MCPT_E_INVALID, "NULL argument");
    out->n_geometries = static_cast<int64_t>(s->hs.geoms.size());
    out->n_triangles = static_cast<int64_t>(s->hs.kd_tris.size());
    out->n_nodes = static_cast<int64_t>(s->hs.nodes.size());
    out->n_leaf_refs = static_cast<int64_t>(s->hs.leaf_ids.size());
    out->kd_depth = s->hs.kd_depth;
    out->lds_bytes = s->gpu.node_boxes ? 0 : s->gpu.image_bytes;
    out->node_boxes = s->gpu.node_boxes;
    out->device = s->device;
    out->n_devices = s->on_device ? 1 + static_cast<int64_t>(s->replicas.size()) : 0;
    out->kd_build = s->hs.kd_build;
    return MCPT_OK;
}

int mcpt_scene_primary_tile_classes(mcpt_scene* s, uint32_t out[4]) {
    if (!s || !out) return MCPT_E_INVALID;
    return guarded([&] {
        out[0] = out[1] = out[2] = 0;
        out[3] = mcpt::kListK;
        if (!s->on_device || !s->ws.small.p) return MCPT_OK;
        set_device(*s);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, tile_classes(*s), 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return MCPT_OK;
    });
}

int mcpt_scene_terminal_cull_boxes(const mcpt_scene* s) {
    return s ? static_cast<int>(s->tables.n_cull_boxes) : 0;
}

int mcpt_scene_miss_cull_boxes(const mcpt_scene* s, float* boxes) {
    if (!s) return 0;
    if (boxes) std::memcpy(boxes, s->tables.miss_box, sizeof(float) * 6 * s->tables.n_miss_boxes);
    return static_cast<int>(s->tables.n_miss_boxes);
}

int mcpt_scene_direct_lists(const mcpt_scene* s, int32_t* tri_box, uint32_t* box_tris, uint32_t* lists,
                            int32_t* list_kd) {
    if (!s) return 0;
    const RouteTables& t = s->tables;
    if (list_kd)
        for (uint32_t b = 0; b < mcpt::kMaxMissBoxes; ++b)
            for (uint32_t j = 0; j < mcpt::kDirectK; ++j) {
                const bool have = j < ((t.direct_counts >> (4u * b)) & 15u);
                list_kd[b * mcpt::kDirectK + j] =
                    have ? static_cast<int32_t>(s->tri_order[t.direct_list[b * mcpt::kDirectK + j] / 3u]) : -1;
            }
    if (tri_box && !t.tri_box.empty()) std::memcpy(tri_box, t.tri_box.data(), 4 * t.tri_box.size());
    if (box_tris) std::memcpy(box_tris, t.box_tris, 4 * mcpt::kMaxMissBoxes);
    if (lists) std::memcpy(lists, t.direct_list, 4 * mcpt::kDirectTableWords);
    return static_cast<int>(mcpt::kDirectK);
}

uint64_t mcpt_scene_direct_rays(const mcpt_scene* s) { return s ? s->routes.direct_rays : 0; }
uint64_t mcpt_scene_extend_rays(const mcpt_scene* s) { return s ? s->routes.extend_rays : 0; }
uint64_t mcpt_scene_clipped_rays(const mcpt_scene* s) { return s ? s->routes.clipped_rays : 0; }
uint64_t mcpt_scene_primary_shaded(const mcpt_scene* s) { return s ? s->routes.primary_shaded : 0; }
uint64_t mcpt_scene_sphere_skips(const mcpt_scene* s) { return s ? s->routes.sphere_skips : 0; }
uint32_t mcpt_scene_clip_spheres(const mcpt_scene* s, float* spheres) {
    if (!s) return 0;
    if (spheres) std::memcpy(spheres, s->tables.clip_sphere, sizeof s->tables.clip_sphere);
    return s->tables.clip_spheres;
}
uint64_t mcpt_scene_primary_shade_lds(const mcpt_scene* s) {
    if (!s) return 0;
    mcpt::WfFacts f = scene_facts(*s);   // (a lean render's route: the lists as it turns them on)
    f.lean = true;
    return mcpt::wf_route(f).primary_shade_lds;
}

int mcpt_scene_copy_kd(const mcpt_scene* s, uint32_t* nodes, uint32_t* leaf_ids, int32_t* kd_tris, float* geoms) {
    if (!s) return fail(MCPT_E_INVALID, "NULL scene");
    const auto& hs = s->hs;
    if (nodes)
        for (size_t i = 0; i < hs.nodes.size(); ++i) {
            const auto& n = hs.nodes[i];
            uint32_t* o = nodes + 12 * i;
            o[0] = n.left; o[1] = n.right; o[2] = n.axis;
            std::memcpy(&o[3], &n.split, 4);
            std::memcpy(&o[4], n.bmin, 12);
            std::memcpy(&o[7], n.bmax, 12);
            o[10] = n.leaf_begin; o[11] = n.leaf_count;
        }
    if (leaf_ids && !hs.leaf_ids.empty()) std::memcpy(leaf_ids, hs.leaf_ids.data(), hs.leaf_ids.size() * 4);
    if (kd_tris) std::memcpy(kd_tris, hs.kd_tris.data(), hs.kd_tris.size() * 4);
    if (geoms)
        for (size_t g = 0; g < hs.geoms.size(); ++g) {
            const auto& e = hs.geoms[g];
            float* o = geoms + 14 * g;
            o[0] = e.Ka.x; o[1] = e.Ka.y; o[2] = e.Ka.z; o[3] = e.Kd.x; o[4] = e.Kd.y; o[5] = e.Kd.z;
            o[6] = e.Ks.x; o[7] = e.Ks.y; o[8] = e.Ks.z; o[9] = e.Ns; o[10] = e.Tr; o[11] = e.Ni;
            o[12] = static_cast<float>(e.start); o[13] = static_cast<float>(e.count);
        }
    return MCPT_OK;
}

}  // extern "C"
