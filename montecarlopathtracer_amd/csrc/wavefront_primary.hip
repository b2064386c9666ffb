// wavefront_primary.hip -- the wavefront pipeline's bounce-0 kernels for scenes
// in LDS: the packet extend wf_extend_primary and its primary-list form
// wf_primary_lists, with their launches (called by wavefront.hip's
// launch_wavefront).  A translation unit of its own so that it can take its own
// code-generation flags (_build.py: wave-uniform control flow left
// unstructurized); what it shares with wavefront.hip is wf_device.hpp.
// wf_primary_shade, the list form that also shades bounce 0, is in a sibling
// translation unit, wavefront_primary_shade.hip (other flags, and this file's
// kernels keep their code); it shares the walk and the listed groups' pair
// tests with the kernels here as source text: wf_primary_walk.hpp and
// wf_primary_pairs.hpp, both included by wf_primary_body.hpp.
#include "wf_device.hpp"

namespace mcpt {
namespace {

// ---- extend of bounce 0, wave-coherent (CV mode, queue-order shade) ---------
// Primary rays share the eye as their origin, and generate deals them in
// 64-path groups -- one 8x8 tile of one sample -- so a wave takes one group
// and walks the KD tree ONCE for its 64 rays: the node is wave-uniform (read
// by one LDS broadcast), each lane keeps its own interval, hit and an active
// flag, and the wave enters a child if any lane's interval reaches it.  With
// a common origin every lane has the same near side at every split plane (an
// origin exactly on the plane leaves only lanes inside the plane needing both
// children, and their near child is the left one), so the wave's front-to-back
// order is each lane's own: a lane is active at exactly the nodes its own
// ordered walk (trav_iter) visits, with the same interval and best hit there,
// and it stops at the same pop.  Hits, visit and test counts are therefore
// those of the per-ray walk, bit for bit; only the schedule differs (one
// wave-uniform descent per node instead of 64 divergent ones).
// Stack: the per-ray walk's lazy LDS stack (S entries in LDS, older ones in
// the spill area) with a wave-uniform position; a lane's copy of an entry
// carries its interval, or tmax = NaN if the lane is not in that subtree.
//
// The kernel's body is wf_primary_body.hpp (the walk itself: wf_primary_walk.hpp,
// which it includes), included once per kernel below:
// source text, not a function, so that wf_extend_primary's code stays what it
// was without the second kernel (inlined from a shared function, its epilogue
// came out one instruction shorter).
// LIST (wf_primary_lists, render_launch.hpp "Primary lists"; lean renders
// whose groups are whole 8x8 tiles): a group first reads its tile's candidate
// record (wf_tile_candidates), fetched one group ahead.  No candidate: every
// lane's ray is a miss, and nothing but the path count is computed.  Up to
// kListK: each lane makes its ray as the walk would (a root-box miss stays a
// miss) and tests the listed triangles two at a time from their LDS records,
// the next pair's indices loaded behind the current pair's tests.  More: the
// packet walk.  (Its name must not contain "wf_extend": the resource pins
// count the kernels that do.)
template <int S, int BLOCK, bool COUNT>
__global__ void __launch_bounds__(BLOCK, 1) wf_extend_primary(const KernelParams kp, const WfParams wf) {
    constexpr bool LIST = false;
#include "wf_primary_body.hpp"
}
// (<= 88 VGPRs, as the LDS scenes' other lean extends: two shade waves per SIMD beside it)
template <int S, int BLOCK>
__global__ void __launch_bounds__(BLOCK, 1) wf_primary_lists(const KernelParams kp, const WfParams wf) {
    constexpr bool LIST = true, COUNT = false;
#include "wf_primary_body.hpp"
}

}  // namespace

hipError_t launch_wavefront_primary(const KernelParams& kp, const WfParams& wf, int grid, size_t lds,
                                    hipStream_t st) {
    auto kern = kp.lean ? wf_extend_primary<4, kLdsBlock, false> : wf_extend_primary<4, kLdsBlock, true>;
    return launch_dyn_lds(kern, dim3(grid), dim3(kLdsBlock), lds, st, kp, wf);
}
hipError_t launch_wavefront_primary_lists(const KernelParams& kp, const WfParams& wf, int grid, size_t lds,
                                          hipStream_t st) {
    return launch_dyn_lds(wf_primary_lists<4, kLdsBlock>, dim3(grid), dim3(kLdsBlock), lds, st, kp, wf);
}

}  // namespace mcpt
