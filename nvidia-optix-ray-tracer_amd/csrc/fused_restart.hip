// fused_restart.hip -- k_path_restart: k_path_one (fused_one.hip) whose repeat primary rays start at the node of their known hit.  The reference's
// raygen has no pixel jitter, so every sample of a pixel sends the same primary ray; since HRT_SEED_PRIMARY=2 such a ray walks inside a window
// under the hit its predecessor found, yet from the root: all but the last node of that walk are the root-to-leaf path the predecessor took,
// one child meeting the window in each.  Here the loop's primitive test keeps the RECORD a hit was accepted from (TravState::binst, which a
// one-group kernel has free), the regeneration looks the record up in the tree's leaf_parent table -- record -> the node whose leaf slot holds
// it -- and the next primary ray starts there (fused_body.h: s_restart; DESIGN.md section 4.1 "The start under the known hit").  Same pixels,
// same random numbers, same ray counts as k_path_one.  A kernel and a translation unit of its own: k_path_one's loop, registers and LDS are
// pinned by tests/test_one_group_cpu.py, and the other kernels' instruction streams are not touched.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

struct RestartVariant : FusedBodyVariant<false> { static constexpr bool kBlocks = true, kOneGroup = true, kRestart = true; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
__global__ __launch_bounds__(kTraverseBlock, HRT_FUSED_WAVES_PER_SIMD) void k_path_restart(TraverseArgs a) {
    fused_body<RestartVariant>(a);
}

// The table: scene.leaf_parent has one word per record of the launch's tree.  It rides in PathArgs::slice_order, which a launch in blocks
// must not have (path_launch_admitted, which has checked the caller's TraverseArgs as it came) and whose place the kernel therefore has
// free: the launch gets a copy with the table in it.
void launch_path_restart(const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s) {
    TraverseArgs b = a;
    b.path.slice_order = scene.leaf_parent;
    hipLaunchKernelGGL(k_path_restart, dim3(grid_blocks), dim3(kTraverseBlock), 0, s, b);
}

}  // namespace hrt
