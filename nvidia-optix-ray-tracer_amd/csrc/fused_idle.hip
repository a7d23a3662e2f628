// fused_idle.hip -- k_path_idle: k_path_restart (fused_restart.hip) whose loop switches the lanes without work off for the primitive test and the
// node step.  Since round 5 both run for the whole wave on whatever the landing registers hold, and a lane without a record / a node rejects
// the outcome afterwards: no mask save, branch or restore -- and, on the C4 frame, about 44 of 64 lanes of the primitive test and 12 of 64 of
// the node step computing nothing (tools/lane_stats.py).  Here the two masks the loop already carries in scalar registers (mask_p, mask_n0)
// and already sets for its loads stay in exec for those two stretches: five moves to exec per iteration where k_path_restart has four,
// one scalar `and` less, nothing saved, no branch -- the same 402 instructions (trav_loop.h: kIdleOff, with the argument why every lane is
// active where the moves are made; trav_lean.h: the moves).  Same pixels, same random numbers, same ray counts, same bits as k_path_restart:
// what is not computed was never used.  The point is energy, not instructions: a quarter fewer active lane-operations per iteration, which the
// chip returns as clock -- 2250 -> 2320 MHz under this kernel on C4, +1.2 % in time (profiles/r29_idle_lanes.txt).
// A kernel and a translation unit of its own: k_path_restart's loop, registers and LDS are pinned by tests/test_primary_restart_cpu.py, and
// the other kernels' instruction streams are not touched.  PathKernel::MaskIdle (device_types.h); k_path_direct, which is this kernel plus
// one flag, has its own enumerator, unit and launcher (fused_direct.hip).
#include "fused_body.h"

#pragma clang fp contract(off)

namespace hrt {

struct MaskIdleVariant : FusedBodyVariant<false> { static constexpr bool kBlocks = true, kOneGroup = true, kRestart = true, kMaskIdle = true; };
// (the TraverseArgs must stay the ONLY explicit argument, at offset 0 of the kernel-argument segment: the regeneration reads its constants
// from the segment itself, fused_body.h: kernarg_traverse_args)
__global__ __launch_bounds__(kTraverseBlock, HRT_FUSED_WAVES_PER_SIMD) void k_path_idle(TraverseArgs a) {
    fused_body<MaskIdleVariant>(a);
}

// (the leaf_parent table rides in PathArgs::slice_order, as in launch_path_restart)
void launch_path_idle(const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s) {
    TraverseArgs b = a;
    b.path.slice_order = scene.leaf_parent;
    hipLaunchKernelGGL(k_path_idle, dim3(grid_blocks), dim3(kTraverseBlock), 0, s, b);
}

}  // namespace hrt
