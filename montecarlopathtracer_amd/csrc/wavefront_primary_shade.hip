// wavefront_primary_shade.hip -- wf_primary_shade, the wavefront pipeline's bounce-0
// kernel that resolves its groups as wf_primary_lists does and shades them in
// place (render_launch.hpp "Primary shade"), with its launch (called by
// wavefront.hip's launch_wavefront).  A translation unit of its own: beside
// wavefront_primary.hip's kernels wf_primary_lists came out one instruction
// longer, and its instruction stream is pinned; and it takes wavefront.hip's
// flags, not the packet extend's -- with wave-uniform regions left unstructurized
// the divergent per-item code was miscompiled (emitter hits beside scattering
// lanes stored zero) -- with the register-minimising scheduler (_build.py).  It
// shares the packet walk with the packet extends as source text
// (wf_primary_walk.hpp) and the path rule with wf_shade_slots (wf_shade_item.hpp).
#include "wf_device.hpp"

namespace mcpt {
namespace {

// The lean renders that wf_primary_lists serves and whose queue-order shade culls
// and carries (WfParams::shade_cull): a group is resolved the same way -- empty
// record, pair tests or the packet walk -- and then shaded by the lanes that
// hold it, through the shade's own per-item code: no hit id is stored, bounce 0
// has no shade launch, and a tile without a candidate gets its zeros here.  The
// body is wf_primary_shade_body.hpp.  (The name must contain neither
// "wf_primary_lists" nor "wf_extend": the resource pins match kernels by those.)
// Held at <= 88 VGPRs (amdgpu_num_vgpr counts half of gfx950's unified file: 44) and the lean LDS extend's LDS, its direct table included:
// the other stream's 512-thread shade still runs two waves per SIMD beside it.
template <int S, int BLOCK>
__global__ void __launch_bounds__(BLOCK, 1) __attribute__((amdgpu_num_vgpr(44)))
wf_primary_shade(const KernelParams kp, const WfParams wf) {
#include "wf_primary_shade_body.hpp"
}

}  // namespace

hipError_t launch_wavefront_primary_shade(const KernelParams& kp, const WfParams& wf, int grid, size_t lds,
                                          hipStream_t st) {
    return launch_dyn_lds(wf_primary_shade<4, kLdsBlock>, dim3(grid), dim3(kLdsBlock), lds, st, kp, wf);
}

}  // namespace mcpt
