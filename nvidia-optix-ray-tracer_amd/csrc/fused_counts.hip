// fused_counts.hip -- k_path_counts: the persistent path kernel (fused_body.h) in which every pixel takes a sample count of its own and
// continues a sum the caller keeps, in frame order (path_lane.h: path_take / path_finish, kCounts; hrt_render_accumulate, DESIGN.md section
// 2.1 "Per-pixel sample counts").  The launches k_fused<S, I, false> would run otherwise -- no primary-hit cache, no sample blocks, no capture --
// for one-level and two-level trees.  Kernels and a translation unit of their own: k_fused (fused.hip), k_path_blocks (fused_blocks.hip) and
// the others, whose registers, spills and loops the tests pin, know neither the counts nor the fourth accumulator.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

template <bool HAS_SPHERES, bool INSTANCED>
struct CountsVariant : FusedBodyVariant<false> { static constexpr bool kSpheres = HAS_SPHERES, kInstanced = INSTANCED, kCounts = true; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
template <bool HAS_SPHERES, bool INSTANCED>
__global__ __launch_bounds__(kTraverseBlock, INSTANCED ? HRT_INST_WAVES_PER_SIMD : HRT_FUSED_WAVES_PER_SIMD) void k_path_counts(TraverseArgs a) {
    fused_body<CountsVariant<HAS_SPHERES, INSTANCED>>(a);
}

// a.path.accum / trace_inst: width * height sums and sample totals in frame order; a.path.slice_order: as many counts, or NULL; a.path.trace_rays,
// slice_cost, primary_cache and sample_block are not set (path_launch_admitted)
void launch_path_counts(const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s) {
    const dim3 g(grid_blocks), b(kTraverseBlock);
    switch ((scene.has_spheres ? 2 : 0) | (scene.one_level ? 0 : 1)) {
        case 0: hipLaunchKernelGGL((k_path_counts<false, false>), g, b, 0, s, a); break;
        case 1: hipLaunchKernelGGL((k_path_counts<false, true>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_path_counts<true, false>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((k_path_counts<true, true>), g, b, 0, s, a); break;
    }
}

}  // namespace hrt
