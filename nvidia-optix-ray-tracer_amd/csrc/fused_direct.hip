// fused_direct.hip -- k_path_direct: k_path_idle (fused_idle.hip) whose repeat primary rays are decided where they are made.  The reference has no
// pixel jitter, so every sample's primary ray is the same ray and ends in the same hit; since k_path_restart such a ray walked 1.01 to 1.03 node
// visits and 1.48 primitive tests from the node of its known hit -- alive for two or three iterations of its wave, then waiting half a
// regeneration period to be shaded in a second regeneration.  Here the lane's word holds the RECORD its pixel's last primary ray accepted its
// hit from, and the regeneration that starts the pixel's next sample fetches that record (48 bytes) and runs the canonical primitive test on it
// with the culling bound at the seed: the identical ray recomputes the identical t, u, v, and a complete walk has shown that no primitive
// computes a smaller (t, primitive id).  The lane is shaded in the same pass and launches its bounce; the ray is still launched and counted,
// fetches its primitive and is decided by the canonical test against the launch's tmin and tmax (fused_body.h: kDirect; DESIGN.md sections 2.1
// and 4.1).  The traversal loop is k_path_idle's, instruction for instruction: everything new is in the regeneration.  Same pixels, same random
// numbers, same ray counts, same bits.  A kernel and a translation unit of its own: the other kernels' instruction streams are not touched.
// PathKernel::Direct (device_types.h): chosen where k_path_idle would be and HRT_PRIMARY_DIRECT is on, launched by the one entry like the rest.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

// k_path_idle's variant (fused_idle.hip: MaskIdleVariant, flag for flag) plus kDirect
struct DirectVariant : FusedBodyVariant<false> { static constexpr bool kBlocks = true, kOneGroup = true, kRestart = true, kMaskIdle = true, kDirect = true; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
__global__ __launch_bounds__(kTraverseBlock, HRT_FUSED_WAVES_PER_SIMD) void k_path_direct(TraverseArgs a) {
    fused_body<DirectVariant>(a);
}

// (k_path_direct reads no table; the tree's leaf_parent rides along as in launch_path_idle, so that the two launches differ in the kernel alone)
void launch_path_direct(const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s) {
    TraverseArgs b = a;
    b.path.slice_order = scene.leaf_parent;
    hipLaunchKernelGGL(k_path_direct, dim3(grid_blocks), dim3(kTraverseBlock), 0, s, b);
}

}  // namespace hrt
