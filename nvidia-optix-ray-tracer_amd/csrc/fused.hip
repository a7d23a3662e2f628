// fused.hip -- k_fused, the production kernel of hrt_render_launch: the whole render in ONE persistent launch.
//
// Replaces the OptiX launch of the reference (raygen -> optixTrace -> closest-hit / miss, recursively, shader/Shader.cu:46-287;
// launched at src/Global/RendererMesh.cu:416-419).  Same execution model as round 1's fused mode of k_traverse (kernels.hip,
// still there for trees beyond k_fused's limits): every lane OWNS a pixel and carries its path state in registers -- RNG state, sample and depth
// counters, the albedo chain, the running sum; waves take 16-pixel slices of the tile from sharded counters; a lane whose ray
// has finished waits, and once enough lanes of the wave wait a regeneration phase (wave-uniform branch) shades them in place
// with the shared device functions of trav_common.h and starts the next ray in the same lane: the bounce, the next sample's
// primary ray, or the next pixel.  No ray queues, no hit records, no stage barriers.
// What is new: the traversal step between two regenerations -- trav_lean.h, written for instruction
// count: the SIMD issues one instruction of any kind per ~2.4 cycles and this kernel is bound by exactly that --, one scatter body
// for all programs, an issue priority per loop phase, and tail splitting once the tile is used up (lanes without a pixel take
// subtrees off the busy lanes' stacks; the pieces of a ray share one best hit in LDS).  The loop between two regenerations is
// trav_loop.h's, shared with k_trace_queue (fused_queue.hip); the steps of the regeneration phase are path_lane.h's, shared with
// k_traverse<.., FUSED>.  What is here is when a regeneration happens, the primary-hit cache (kReuse) round those steps, and the
// two-level tree's transform-node steps -- and launch_path_kernel, the one way every path kernel is launched.
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

template <bool HAS_SPHERES, bool INSTANCED, bool REUSE>
struct FusedVariant : FusedBodyVariant<REUSE> { static constexpr bool kSpheres = HAS_SPHERES, kInstanced = INSTANCED; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
template <bool HAS_SPHERES, bool INSTANCED, bool REUSE>
__global__ __launch_bounds__(kTraverseBlock, INSTANCED ? HRT_INST_WAVES_PER_SIMD : HRT_FUSED_WAVES_PER_SIMD) void k_fused(TraverseArgs a) {
    fused_body<FusedVariant<HAS_SPHERES, INSTANCED, REUSE>>(a);
}

// one launch renders every sample of every pixel of the tile: the instantiation for the scene's primitives and, where the caller has set
// a primary-hit cache up, primary reuse
template <bool INSTANCED>
static void launch_fused_as(const TraverseArgs &a, bool has_spheres, uint32_t grid_blocks, hipStream_t s) {
    const dim3 g(grid_blocks), b(kTraverseBlock);
    switch ((has_spheres ? 2 : 0) | (a.path.primary_cache != nullptr ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((k_fused<false, INSTANCED, false>), g, b, 0, s, a); break;
        case 1: hipLaunchKernelGGL((k_fused<false, INSTANCED, true>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_fused<true, INSTANCED, false>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((k_fused<true, INSTANCED, true>), g, b, 0, s, a); break;
    }
}

// The one way a path kernel is launched: the launch is held to what the kernel the caller names takes for granted, and that kernel's own translation unit
// launches it.  Every kernel has its enumerator and its case: no launcher forwards to another kernel, and no argument doubles as a selector.
bool launch_path_kernel(PathKernel kernel, const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s) {
    if (!path_launch_admitted(kernel, a, scene, grid_blocks)) return false;
    switch (kernel) {
        case PathKernel::Fused: launch_fused_as<false>(a, scene.has_spheres, grid_blocks, s); break;
        case PathKernel::FusedInstanced: launch_fused_as<true>(a, scene.has_spheres, grid_blocks, s); break;      // (transform nodes over shared BLASes)
        case PathKernel::Capture: launch_path_capture(a, scene, grid_blocks, s); break;
        case PathKernel::Blocks: launch_path_blocks(a, scene, grid_blocks, s); break;
        case PathKernel::OneGroup: launch_path_one(a, scene, grid_blocks, s); break;
        case PathKernel::Restart: launch_path_restart(a, scene, grid_blocks, s); break;
        case PathKernel::MaskIdle: launch_path_idle(a, scene, grid_blocks, s); break;
        case PathKernel::Direct: launch_path_direct(a, scene, grid_blocks, s); break;
        case PathKernel::Round1: launch_path_round1(a, scene, grid_blocks, s); break;
        case PathKernel::Counts: launch_path_counts(a, scene, grid_blocks, s); break;
    }
    return true;
}

}  // namespace hrt
