// fused_blocks.hip -- k_path_blocks: the persistent path kernel (fused_body.h) handing pixels out in sample blocks (path_lane.h; DESIGN.md
// section 2.1).  A kernel and a translation unit of its own: the hand-over costs the regeneration ten spilled registers (lane state), which k_fused
// (fused.hip) -- whose registers, spills and loop tests/test_host_cpu.py pins -- need not pay.  One-level trees, no primary-hit cache.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

template <bool HAS_SPHERES>
struct BlocksVariant : FusedBodyVariant<false> { static constexpr bool kSpheres = HAS_SPHERES, kBlocks = true; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
template <bool HAS_SPHERES>
__global__ __launch_bounds__(kTraverseBlock, HRT_FUSED_WAVES_PER_SIMD) void k_path_blocks(TraverseArgs a) {
    fused_body<BlocksVariant<HAS_SPHERES>>(a);
}

// (what the kBlocks instantiations take for granted -- a render in sample blocks, with no callers' rays, no cost probe and no slice order,
// fields their regeneration does not look at -- every launch is held to before it gets here: device_types.h, path_launch_admitted)
void launch_path_blocks(const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s) {
    const dim3 g(grid_blocks), b(kTraverseBlock);
    if (scene.has_spheres) hipLaunchKernelGGL((k_path_blocks<true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_path_blocks<false>), g, b, 0, s, a);
}

}  // namespace hrt
