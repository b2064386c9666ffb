// The wavefront's route and batch split (csrc/wf_route.hpp), printed for
// tests/test_wf_route_cpu.py to check implications on:
//   C key=value ...   the header's constants
//   R key=value ...   the route over a grid of scene and render facts
//   N name key=...    the routes the GPU suite pins by counters, for a scene01-sized scene
//   S key=value ...   a batch split, followed by its batches:
//   B chunk_index s_begin nsc ns v0 nb seg nb_max   (wf_batch_params' fields, and the span's nb_max)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../montecarlopathtracer_amd/csrc/wf_route.hpp"

using namespace mcpt;

namespace {

constexpr int kCus = 256;
constexpr uint32_t kStack4 = 4u * kLdsBlock * 16u;

void print_route(const WfFacts& f, const WfRoute& r) {
    const GpuScene& sc = *f.scene;
    std::printf("lean=%d sort=%d qe=%d listed=%d tile=%d default_batch=%d n_miss=%u counts=%u n_cull=%u n_tris=%u "
                "image=%u node_boxes=%u n_geoms=%u max_depth=%d cus=%d ",
                f.lean, f.sort, f.qe, f.listed, f.tile, f.default_batch, f.n_miss_boxes, f.direct_counts,
                f.n_cull_boxes, sc.n_tris, sc.image_bytes, sc.node_boxes, sc.n_geoms, f.max_depth, f.cus);
    std::printf("in_lds=%d nseg=%u variant=%d queries=%d terminal=%d r_miss=%u r_counts=%u direct=%d shade_cull=%d "
                "carry=%d packet=%d generate=%d can_list=%d whole=%d primary_shade=%d cull_bounce=%d group_shift=%u "
                "xcd_deal=%u packet_lds=%zu extend_lds=%zu direct_lds=%zu primary_shade_lds=%zu geo_lds=%zu "
                "shade_block1=%d shade_block2=%d\n",
                r.in_lds, r.nseg, r.variant, r.queries, r.terminal, r.n_miss_boxes, r.direct_counts, r.direct,
                r.shade_cull, r.carry, r.packet, r.generate, r.can_list, r.whole, r.primary_shade, r.cull_bounce,
                r.group_shift, r.xcd_deal, r.packet_lds, r.extend_lds, r.direct_lds, r.primary_shade_lds, r.geo_lds,
                wf_shade_block(r, 1), wf_shade_block(r, 2));
}

// geometries whose material table still fits beside the extend's workgroups and the shade's static LDS
long geo_limit(const WfRoute& r) {
    const size_t ext_cu = r.in_lds ? r.extend_lds : kWfGlobalSegsPerCu * r.extend_lds;
    return (long(kLdsPerCu) - long(ext_cu) - long(kShadeStaticLds)) / 64;
}

KernelParams frame(uint32_t npix, uint32_t spp, uint32_t chunk) {
    KernelParams kp{};
    kp.npix_local = npix;
    kp.spp = spp;
    kp.chunk = std::min(chunk, spp);
    kp.nchunks = (spp + kp.chunk - 1) / kp.chunk;
    return kp;
}

void grid() {
    // the largest image beside which the direct lists fit (images are whole 16-B units)
    const uint32_t fit = uint32_t(kMaxLds - kShadeStaticLds - kDirectLdsBytes - kLdsCounterBytes - kStack4) & ~15u;
    struct Image {
        uint32_t bytes, node_boxes;
    };
    // small; the two sides of direct_lists_fit; a small image forced into global memory; a large one
    const Image images[] = {{40000u, 0u}, {fit, 0u}, {fit + 16u, 0u}, {40000u, 1u}, {1u << 24, 1u}};
    std::printf("C kMaxLds=%zu kLdsPerCu=%zu kLdsCounterBytes=%zu kDirectLdsBytes=%zu kShadeStaticLds=%zu stack4=%u "
                "kWfGlobalSegsPerCu=%d kListMaxTris=%u fit=%u global_lds=%zu\n",
                kMaxLds, kLdsPerCu, kLdsCounterBytes, kDirectLdsBytes, kShadeStaticLds, kStack4, kWfGlobalSegsPerCu,
                kListMaxTris, fit, lds_bytes_global(MCPT_WF_GLOBAL_S, true));
    for (const Image& im : images)
        for (int bits = 0; bits < (1 << 10); bits++) {
            GpuScene sc{};
            sc.image_bytes = im.bytes;
            sc.node_boxes = im.node_boxes;
            sc.n_tris = (bits & 1) ? kListMaxTris + 1u : kListMaxTris;
            sc.n_geoms = 1;
            WfFacts f{};
            f.scene = &sc;
            f.cus = kCus;
            f.lean = bits & 2;
            f.sort = bits & 4;
            f.qe = bits & 8;
            f.listed = bits & 16;
            f.tile = (bits & 32) ? 4 : 8;
            f.default_batch = bits & 64;
            f.n_miss_boxes = (bits & 128) ? 8u : 0u;
            f.direct_counts = (bits & 256) ? 0x22222u : 0u;
            f.n_cull_boxes = (bits & 512) ? 1u : 0u;
            f.tile_records = f.tile == 8;
            f.max_depth = 3;
            f.group_shift = 12;
            const long lim = std::max(geo_limit(wf_route(f)), 1L);
            for (long g : {lim, lim + 1}) {
                sc.n_geoms = uint32_t(g);
                std::printf("R geo_limit=%ld ", geo_limit(wf_route(f)));
                print_route(f, wf_route(f));
            }
        }
}

// a 64 x 64 frame of scene01 (3 spp in chunks of 2, depth 3), as the GPU suite renders it
void named() {
    GpuScene sc{};
    sc.image_bytes = 40000u;
    sc.n_tris = 900;
    sc.n_geoms = 9;
    WfFacts base{};
    base.scene = &sc;
    base.cus = kCus;
    base.lean = true;
    base.tile = 8;
    base.tile_records = true;
    base.default_batch = true;
    base.n_miss_boxes = 8;
    base.direct_counts = 0x22222u;
    base.n_cull_boxes = 1;
    base.max_depth = 3;
    base.group_shift = 12;
    const KernelParams kp = frame(4096, 3, 2);
    // the default batch of that frame on two streams: half its 3 x 4096 paths
    auto row = [&](const char* name, const WfFacts& f, uint32_t capacity) {
        const WfRoute r = wf_route(f);
        const bool lists = r.can_list && any_whole_tile_batch(kp, capacity, r.whole);
        std::printf("N %s lists=%d fused=%d ", name, lists, lists && r.primary_shade);
        print_route(f, r);
    };
    WfFacts f = base;
    row("default", f, 6144);
    f = base; f.sort = true;
    row("sorted", f, 6144);
    f = base; f.tile = 4; f.tile_records = false;
    row("tile4", f, 6144);
    f = base; f.default_batch = false;
    row("batch200", f, 200);
    f = base; f.qe = true;
    row("qe", f, 6144);
    f = base; f.listed = true;
    row("listed", f, 6144);
    f = base; f.lean = false;
    row("counting", f, 6144);
}

void splits() {
    GpuScene sc{};
    sc.image_bytes = 40000u;
    WfFacts f{};
    f.scene = &sc;
    f.cus = kCus;
    const WfRoute r = wf_route(f);
    std::printf("C split_nseg=%u split_group_shift=%u\n", r.nseg, r.group_shift);
    for (uint32_t npix : {64u, 192u, 3072u})
        for (uint32_t spp : {1u, 3u, 8u})
            for (uint32_t chunk : {1u, 2u, 3u}) {
                if (chunk > spp) continue;   // (the plan clamps it: the same frame as chunk = spp)
                const KernelParams kp = frame(npix, spp, chunk);
                const uint64_t unit = uint64_t(npix) * chunk, work = uint64_t(npix) * spp;
                std::vector<uint64_t> caps = {chunk, 64, 100, 64ull * chunk, 200, 1000, unit - 1, unit, unit + 1,
                                              2 * unit, work - 1, work};
                std::sort(caps.begin(), caps.end());
                caps.erase(std::unique(caps.begin(), caps.end()), caps.end());
                for (uint64_t cap : caps) {
                    if (cap < chunk || cap > work) continue;   // (wf_batch_capacity keeps a batch inside these)
                    if (cap < 64 && npix > 192) continue;      // (one pixel per batch: the smaller frames show it)
                    for (int whole = 0; whole < 2; whole++) {
                        std::printf("S npix=%u spp=%u chunk=%u nchunks=%u capacity=%u whole=%d any_whole=%d\n", npix, spp,
                                    kp.chunk, kp.nchunks, uint32_t(cap), whole,
                                    any_whole_tile_batch(kp, uint32_t(cap), whole != 0));
                        wf_for_each_batch(kp, uint32_t(cap), whole != 0, [&](const WfSpan& s, uint32_t chunk0, uint32_t v0) {
                            const WfParams w = wf_batch_params(WfParams{}, r, kp, s, chunk0, v0);
                            std::printf("B %u %u %u %u %u %u %u %u\n", w.chunk_index, w.s_begin, w.nsc, w.ns, w.v0, w.nb,
                                        w.seg, s.nb_max);
                            return true;
                        });
                    }
                }
            }
}

}  // namespace

int main() {
    grid();
    named();
    splits();
    return 0;
}
