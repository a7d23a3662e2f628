// fused_one.hip -- k_path_one: k_path_blocks (fused_blocks.hip) for a scene with ONE hit group -- a one-level tree of triangles over exactly
// one instance, which is what a single-mesh render is.  Every table the path kernels index by the instance that
// was hit -- hitgroups, inst_program, the albedo chain of a path -- has one entry there, entry 0, so the kOneGroup instantiation of the
// shared code (fused_body.h, path_lane.h, trav_loop.h, trav_common.h) reads it with scalar loads where it is used, keeps no chain, and
// decides the primitive test's ties by the primitive id alone.  Same pixels, same random numbers, same ray counts as k_path_blocks<false>.
// A kernel and a translation unit of its own, like k_path_blocks: the other kernels' instruction streams are not touched.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

struct OneGroupVariant : FusedBodyVariant<false> { static constexpr bool kBlocks = true, kOneGroup = true; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
__global__ __launch_bounds__(kTraverseBlock, HRT_FUSED_WAVES_PER_SIMD) void k_path_one(TraverseArgs a) {
    fused_body<OneGroupVariant>(a);
}

// (what the instantiation takes for granted on top of k_path_blocks' facts -- every hit is instance 0's: a one-level tree of triangles over
// exactly one instance -- every launch is held to before it gets here: device_types.h, path_launch_admitted)
void launch_path_one(const TraverseArgs &a, const PathScene &, uint32_t grid_blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_path_one, dim3(grid_blocks), dim3(kTraverseBlock), 0, s, a);
}

}  // namespace hrt
