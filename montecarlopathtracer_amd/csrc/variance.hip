// variance.hip -- per-pixel variance of a render's pixel mean, by batch means
// over the per-chunk partial sums the render already wrote (render.hip /
// wavefront.hip: partial[chunk][pixel], and the megakernel's tail-split buffer).
// The path kernels are untouched; this is one more kernel on the render's stream.
//
//   K    = nchunks (>= 2), n_c = samples of chunk c (the last may be shorter)
//   P_c  = the chunk's partial sum (tail-split units: the in-order sum over the
//          tail buffer, exactly as reduce_kernel forms it)
//   sum  = P_0 + P_1 + ... in chunk order;  mean = sum / (float)spp
//   acc  = sum over c, in chunk order, of (float)n_c * (d * d),
//          d = P_c / (float)n_c - mean
//   var  = acc / ((float)spp * (float)(K - 1))
//   prev_count > 0:  var = ((old * pc) * pc + var) / (pc1 * pc1)
//
// fp32, one rounding per operation of the list above (-ffp-contract=off), so
// tests/_var_ref.py restates it in numpy bit for bit.  The values are linear
// radiance squared in both modes (the QuinEngine gamma is the framebuffer's).
//
// One thread per owned pixel through unit_pixel, as reduce_kernel: per chunk a
// wave reads 64 consecutive float4 (1 KiB) at stride npix_local * 16 B.  The
// kernel streams K x 16 B per pixel twice; the second pass hits in L2 while
// K x 16 B x (pixels in flight) fits there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mcpt_device.hpp"
#include "partial_sum.hpp"
#include "trace_device.hpp"
#include "variance_launch.hpp"

namespace mcpt {

using namespace dev;
using namespace trace;

namespace {

__global__ void __launch_bounds__(256) variance_kernel(const KernelParams kp, float4* __restrict__ var) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= kp.npix_local) return;
    int x, y;
    if (!unit_pixel(kp, v, x, y)) return;
    V3 sum = v3(0, 0, 0);
    for (uint32_t c = 0; c < kp.nchunks; c++)
        sum = vadd(sum, chunk_partial(kp, c, v, min(kp.chunk, kp.spp - c * kp.chunk)));
    const V3 mean = vdiv(sum, (float)kp.spp);
    V3 acc = v3(0, 0, 0);
    for (uint32_t c = 0; c < kp.nchunks; c++) {
        const uint32_t n = min(kp.chunk, kp.spp - c * kp.chunk);
        const float nf = (float)n;
        const V3 d = vsub(vdiv(chunk_partial(kp, c, v, n), nf), mean);
        acc = vadd(acc, v3(nf * (d.x * d.x), nf * (d.y * d.y), nf * (d.z * d.z)));
    }
    V3 r = vdiv(acc, (float)kp.spp * (float)(kp.nchunks - 1u));
    const size_t idx = (size_t)y * (size_t)kp.width + (size_t)x;
    if (kp.prev_count != 0) {
        const float4 old = var[idx];
        const float pc = (float)kp.prev_count, pc1 = (float)(kp.prev_count + 1u);
        const float q = pc1 * pc1;
        r = v3(((old.x * pc) * pc + r.x) / q, ((old.y * pc) * pc + r.y) / q, ((old.z * pc) * pc + r.z) / q);
    }
    var[idx] = make_float4(r.x, r.y, r.z, 0.0f);
}

}  // namespace

hipError_t launch_variance(const KernelParams& kp, float4* var, hipStream_t st) {
    if (!kp.npix_local) return hipSuccess;
    hipLaunchKernelGGL(variance_kernel, dim3((kp.npix_local + 255u) / 256u), dim3(256), 0, st, kp, var);
    return hipGetLastError();
}

}  // namespace mcpt
