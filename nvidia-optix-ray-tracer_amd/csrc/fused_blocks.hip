// fused_blocks.hip -- k_path_blocks: the persistent path kernel (fused_body.h) handing pixels out in sample blocks (path_lane.h; DESIGN.md
// section 2.1).  A kernel and a translation unit of its own: the hand-over costs the regeneration ten spilled registers (lane state), which k_fused
// (fused.hip) -- whose registers, spills and loop tests/test_host_cpu.py pins -- need not pay.  One-level trees, no primary-hit cache.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
template <bool HAS_SPHERES>
__global__ __launch_bounds__(kTraverseBlock, HRT_FUSED_WAVES_PER_SIMD) void k_path_blocks(TraverseArgs a) {
    fused_body<HAS_SPHERES, false, false, true>(a);
}

// What the BLOCKS instantiation takes for granted (path_lane.h: path_finish, path_take, path_primary): a render in sample blocks, with no
// callers' rays, no cost probe and no slice order.  Its regeneration does not look at these fields, so a launch that contradicts them is
// refused here (false: nothing was launched) instead of rendering something else.
bool blocks_launch_admitted(const TraverseArgs &a) {
    return a.path.sample_block != 0u && a.path.trace_rays == nullptr && a.path.slice_cost == nullptr && a.path.slice_order == nullptr;
}

bool launch_fused_blocks(const TraverseArgs &a, bool has_spheres, uint32_t grid_blocks, hipStream_t s) {
    if (!blocks_launch_admitted(a)) return false;
    const dim3 g(grid_blocks), b(kTraverseBlock);
    if (has_spheres) hipLaunchKernelGGL((k_path_blocks<true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_path_blocks<false>), g, b, 0, s, a);
    return true;
}

}  // namespace hrt
