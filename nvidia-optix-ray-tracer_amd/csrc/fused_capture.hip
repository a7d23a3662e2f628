// fused_capture.hip -- k_path_capture: the persistent path kernel (fused_body.h) that also leaves every pixel's primary hit in frame order
// (path_lane.h: path_finish, kCapture; HRT_CTX_CAPTURE_PRIMARY, DESIGN.md section 3e "Guides").  The launches k_fused<S, I, false> would
// run otherwise -- no primary-hit cache, no sample blocks -- for one-level and two-level trees.  Kernels and a translation unit of their
// own: k_fused (fused.hip) and k_path_blocks (fused_blocks.hip), whose registers, spills and loops the tests pin, do not know the store.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

template <bool HAS_SPHERES, bool INSTANCED>
struct CaptureVariant : FusedBodyVariant<false> { static constexpr bool kSpheres = HAS_SPHERES, kInstanced = INSTANCED, kCapture = true; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
template <bool HAS_SPHERES, bool INSTANCED>
__global__ __launch_bounds__(kTraverseBlock, INSTANCED ? HRT_INST_WAVES_PER_SIMD : HRT_FUSED_WAVES_PER_SIMD) void k_path_capture(TraverseArgs a) {
    fused_body<CaptureVariant<HAS_SPHERES, INSTANCED>>(a);
}

// a.path.trace_tuvp / trace_inst: width * height records each; a.path.trace_rays, primary_cache and sample_block are not set (path_launch_admitted)
void launch_path_capture(const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s) {
    const dim3 g(grid_blocks), b(kTraverseBlock);
    switch ((scene.has_spheres ? 2 : 0) | (scene.one_level ? 0 : 1)) {
        case 0: hipLaunchKernelGGL((k_path_capture<false, false>), g, b, 0, s, a); break;
        case 1: hipLaunchKernelGGL((k_path_capture<false, true>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_path_capture<true, false>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((k_path_capture<true, true>), g, b, 0, s, a); break;
    }
}

}  // namespace hrt
