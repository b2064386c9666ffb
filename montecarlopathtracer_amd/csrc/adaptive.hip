// adaptive.hip -- variance-driven adaptive sampling: which pixels get another
// pass, the list of them, and the merge of a listed pass.
// The pass itself is render.hip's pixel-list megakernel.
//
// Selection before pass j (fp32, one rounding per operation, -ffp-contract=off;
// tests/_adaptive_ref.py restates it in numpy), k = (0.2126, 0.7152, 0.0722):
//   sd_c = sqrt(max(var_c, 0))
//   s    = (k.x sd_r + k.y sd_g) + k.z sd_b
//   l    = (k.x fb_r + k.y fb_g) + k.z fb_b
//   over = s > threshold (l + lum_floor)
//   active = count == j  and  (no selection  or  OR of over in the (2r+1)^2 window)
// count == j is "active in pass j - 1" (or "every pixel" while all of them
// are), so no separate active bit is kept.
//
// Compaction, ascending packed (tile-major) order so that neighbouring lanes
// of the list kernel keep neighbouring pixels; no workgroup waits on another:
//   count    one thread per packed pixel; a wave's ballot -> masks[wave], the
//            block's four popcounts -> blocks[block]
//   scan     one workgroup: exclusive scan of blocks[] in place, total at the end
//   scatter  rank = blocks[block] + popcounts of the block's earlier waves +
//            popcount of the lower lanes of its own ballot
//
// Merge of a listed pass: per listed pixel the mean and batch-means variance of
// the pass from its partial sums (partial_sum.hpp, the list's unit layout), then
// exactly reduce_kernel's running mean and variance_kernel's blend.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "adaptive_launch.hpp"
#include "mcpt_device.hpp"
#include "partial_sum.hpp"
#include "trace_device.hpp"

namespace mcpt {

using namespace dev;
using namespace trace;

namespace {

__global__ void __launch_bounds__(256) adaptive_over_kernel(uint32_t npx, const float4* __restrict__ fb,
                                                            const float4* __restrict__ var, float threshold,
                                                            float lum_floor, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npx) return;
    const float4 v = var[i], f = fb[i];
    const float kx = 0.2126f, ky = 0.7152f, kz = 0.0722f;
    const float sr = sqrt_rn(fmaxf(v.x, 0.0f)), sg = sqrt_rn(fmaxf(v.y, 0.0f)), sb = sqrt_rn(fmaxf(v.z, 0.0f));
    const float s = (kx * sr + ky * sg) + kz * sb;
    const float l = (kx * f.x + ky * f.y) + kz * f.z;
    flags[i] = s > threshold * (l + lum_floor) ? 1u : 0u;
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptive_count_kernel(const KernelParams kp, const AdaptiveSelect sel,
                                                                        const uint32_t* __restrict__ flags,
                                                                        const uint32_t* __restrict__ count,
                                                                        unsigned long long* __restrict__ masks,
                                                                        uint32_t* __restrict__ blocks) {
    __shared__ uint32_t wave_n[kAdaptiveBlock / 64];
    const uint32_t v = blockIdx.x * (uint32_t)kAdaptiveBlock + threadIdx.x;
    bool a = false;
    int x = 0, y = 0;
    if (v < kp.npix_local && unit_pixel(kp, v, x, y)) {
        a = count[(size_t)y * (size_t)kp.width + (size_t)x] == sel.pass;
        if (a && !sel.all) {
            const int x0 = max(x - sel.radius, 0), x1 = min(x + sel.radius, kp.width - 1);
            const int y0 = max(y - sel.radius, 0), y1 = min(y + sel.radius, kp.height - 1);
            uint32_t any = 0;
            for (int yy = y0; yy <= y1; yy++)
                for (int xx = x0; xx <= x1; xx++) any |= flags[(size_t)yy * (size_t)kp.width + (size_t)xx];
            a = any != 0;
        }
    }
    const unsigned long long m = __ballot(a);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        masks[(size_t)blockIdx.x * (kAdaptiveBlock / 64) + wave] = m;
        wave_n[wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
        for (int w = 0; w < kAdaptiveBlock / 64; w++) n += wave_n[w];
        blocks[blockIdx.x] = n;
    }
}

// exclusive scan of blocks[0 .. n) in place, the total to blocks[n]: one
// workgroup, a contiguous segment per thread, the 256 segment sums scanned in LDS
__global__ void __launch_bounds__(256) adaptive_scan_kernel(uint32_t* __restrict__ blocks, uint32_t n) {
    __shared__ uint32_t sums[256];
    const uint32_t t = threadIdx.x;
    const uint32_t seg = (n + 255u) / 256u;
    const uint32_t b = min(t * seg, n), e = min(b + seg, n);
    uint32_t s = 0;
    for (uint32_t i = b; i < e; i++) s += blocks[i];
    sums[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {
        const uint32_t add = t >= off ? sums[t - off] : 0u;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    uint32_t run = sums[t] - s;   // exclusive prefix of this thread's segment
    for (uint32_t i = b; i < e; i++) {
        const uint32_t c = blocks[i];
        blocks[i] = run;
        run += c;
    }
    if (t == 255u) blocks[n] = sums[255];
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptive_scatter_kernel(const unsigned long long* __restrict__ masks,
                                                                          const uint32_t* __restrict__ blocks,
                                                                          uint32_t* __restrict__ list) {
    const uint32_t v = blockIdx.x * (uint32_t)kAdaptiveBlock + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long* bm = masks + (size_t)blockIdx.x * (kAdaptiveBlock / 64);
    const unsigned long long m = bm[wave];
    if (!((m >> lane) & 1ull)) return;
    uint32_t rank = blocks[blockIdx.x];
    for (uint32_t w = 0; w < wave; w++) rank += (uint32_t)__popcll(bm[w]);
    rank += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    list[rank] = v;
}

__global__ void __launch_bounds__(256) adaptive_merge_kernel(const KernelParams kp, float4* __restrict__ fb,
                                                             float4* __restrict__ var, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= kp.npix_local) return;
    int x, y;
    if (!unit_pixel(kp, kp.pixel_list[i], x, y)) return;   // (listed pixels are inside the image)
    V3 sum = v3(0, 0, 0);
    for (uint32_t c = 0; c < kp.nchunks; c++)
        sum = vadd(sum, chunk_partial(kp, c, i, min(kp.chunk, kp.spp - c * kp.chunk)));
    const V3 mean = vdiv(sum, (float)kp.spp);
    V3 acc = v3(0, 0, 0);
    for (uint32_t c = 0; c < kp.nchunks; c++) {
        const uint32_t n = min(kp.chunk, kp.spp - c * kp.chunk);
        const float nf = (float)n;
        const V3 d = vsub(vdiv(chunk_partial(kp, c, i, n), nf), mean);
        acc = vadd(acc, v3(nf * (d.x * d.x), nf * (d.y * d.y), nf * (d.z * d.z)));
    }
    const V3 r = vdiv(acc, (float)kp.spp * (float)(kp.nchunks - 1u));
    const size_t idx = (size_t)y * (size_t)kp.width + (size_t)x;
    const float pc = (float)kp.prev_count, pc1 = (float)(kp.prev_count + 1u);
    const float q = pc1 * pc1;
    const float4 pv = fb[idx], old = var[idx];
    fb[idx] = make_float4((pv.x * pc + mean.x) / pc1, (pv.y * pc + mean.y) / pc1, (pv.z * pc + mean.z) / pc1, 0.0f);
    var[idx] = make_float4(((old.x * pc) * pc + r.x) / q, ((old.y * pc) * pc + r.y) / q, ((old.z * pc) * pc + r.z) / q,
                           0.0f);
    count[idx] = kp.prev_count + 1u;
}

__global__ void __launch_bounds__(256) adaptive_fill_kernel(uint32_t* __restrict__ count, uint32_t n, uint32_t value) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) count[i] = value;
}

}  // namespace

hipError_t launch_adaptive_select(const KernelParams& kp, const AdaptiveSelect& sel, const AdaptiveWs& ws,
                                  const float4* fb, const float4* var, const uint32_t* count, hipStream_t st) {
    const uint32_t npx = (uint32_t)kp.width * (uint32_t)kp.height;
    const uint32_t nb = adaptive_blocks(kp.npix_local);
    if (!nb) return hipErrorInvalidValue;
    if (!sel.all)
        hipLaunchKernelGGL(adaptive_over_kernel, dim3((npx + 255u) / 256u), dim3(256), 0, st, npx, fb, var,
                           sel.threshold, sel.lum_floor, ws.flags);
    hipLaunchKernelGGL(adaptive_count_kernel, dim3(nb), dim3(kAdaptiveBlock), 0, st, kp, sel, ws.flags, count, ws.masks,
                       ws.blocks);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(256), 0, st, ws.blocks, nb);
    hipLaunchKernelGGL(adaptive_scatter_kernel, dim3(nb), dim3(kAdaptiveBlock), 0, st, ws.masks, ws.blocks, ws.list);
    return hipGetLastError();
}

hipError_t launch_adaptive_merge(const KernelParams& kp, float4* fb, float4* var, uint32_t* count, hipStream_t st) {
    if (!kp.npix_local) return hipSuccess;
    if (!kp.pixel_list || !kp.prev_count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adaptive_merge_kernel, dim3((kp.npix_local + 255u) / 256u), dim3(256), 0, st, kp, fb, var,
                       count);
    return hipGetLastError();
}

hipError_t launch_adaptive_fill(uint32_t* count, size_t n, uint32_t value, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(adaptive_fill_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, count, (uint32_t)n,
                       value);
    return hipGetLastError();
}

}  // namespace mcpt
