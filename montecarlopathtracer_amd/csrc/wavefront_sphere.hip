// wavefront_sphere.hip -- wf_sphere_clip, the wavefront pipeline's secondary extend
// for lean renders of a scene in LDS whose clip walk is active and that has a sphere
// (render_launch.hpp "Sphere clip"; WfRoute::clip), with its launch (called by
// wavefront.hip's launch_wavefront).  It is the lean LDS extend, wf_extend<kLayLds,
// 4, kLdsBlock, false>, with one change in its start-up: a clipped ray's unlisted boxes
// are cut to their spheres (its third kernel argument) before the union.  A
// translation unit of its own with wavefront.hip's flags: that kernel's instruction
// stream is pinned, and the two share their body as source text (wf_extend_body.hpp).
#include "wf_device.hpp"

namespace mcpt {
namespace {

// (The name must not contain "wf_extend": the resource pins count the extends by it.)
// Held at <= 88 VGPRs and the lean LDS extend's LDS: the other stream's 512-thread
// shade still runs two waves per SIMD beside it.
template <int S, int BLOCK>
__global__ void __launch_bounds__(BLOCK, 1)
wf_sphere_clip(const KernelParams kp, const WfParams wf, const SphereClip sphc) {
    constexpr int LAY = kLayLds;
    constexpr bool COUNT = false;
    constexpr bool SPHERE = true;
    constexpr bool RAYS0 = false;
#include "wf_extend_body.hpp"
}

}  // namespace

hipError_t load_wavefront_sphere_clip() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(wf_sphere_clip<4, kLdsBlock>));
}

hipError_t launch_wavefront_sphere_clip(const KernelParams& kp, const WfParams& wf, const SphereClip& clip, int grid,
                                        size_t lds, hipStream_t st) {
    return launch_dyn_lds(wf_sphere_clip<4, kLdsBlock>, dim3(grid), dim3(kLdsBlock), lds, st, kp, wf, clip);
}

}  // namespace mcpt
